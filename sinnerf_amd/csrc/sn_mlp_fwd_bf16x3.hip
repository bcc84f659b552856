// sn_mlp_fwd_bf16x3.hip -- fused NeRF MLP forward at FP32-LEVEL accuracy on the bf16 matrix cores (SN_DTYPE_BF16X3, inference).
//
// The fp32 kernel (sn_mlp_fwd.hip) is pinned at 0.90 of the 157 TF fp32 MFMA peak; the bf16 MFMA is 16x faster.  SURVEY §7
// "Hard parts" sanctions the classic 3-term split for the fp32 configuration:
//     W = Wh + Wl,  x = xh + xl    (h = RNE to bf16, l = RNE to bf16 of the remainder: 16 mantissa bits each)
//     W.x ~= Wh.xh + Wl.xh + Wh.xl            (the dropped Wl.xl is 2^-16 relative per product)
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16 -- three bf16 MFMAs (3 x 32 cycles) instead of eight fp32 ones (8 x 64) per
// 16 k.  Same algorithm and reference lines as the other forward kernels (rendering.py:187-212, 284-285; nerf.py:36-41,
// 122-148); measured error of the whole MLP ~1e-5 norm-wise (fp32: 5e-7, bf16 x 1: 6e-3), two orders inside the fp32 bars
// (tests/test_bf16x3_gpu.py holds it to the reference-generated golden vectors at the FP32 tolerances).
//
// What differs from sn_mlp_fwd_bf16.hip:
// * a wave owns ONE 32-point tile (the AGPR file holds two activation sets x (hi + lo) x 64 registers = 256);
// * weights stream as slabs of K x 128 B: per k-step the hi fragment then the lo fragment (csrc/sn_layout.h DT_BF16X3) through
//   the fp32 kernel's 3-slot ring of 40 KB slots;
// * per k-step three MFMAs on TWO accumulator chains in strict alternation (A B A | B A B | ...): consecutive MFMAs never
//   depend on each other; chain A starts from the bias, chain B from the inline constant 0, the epilogue adds them;
// * the epilogue splits each fp32 result into its (hi, lo) bf16 pair for the next layer's B operands; the embeddings are the
//   EXACT ones of the fp32 kernel (no angle doubling) split the same way; heads in fp32 on the VALU as everywhere.
// STORE (training forward, SN_DTYPE_BF16X3 of sn_mlp_forward_train): additionally writes the training state in the "x3 state" layout of
// sn_layout.h -- NOT the array SN_DTYPE_F32 writes, although it has the same shape and size: slots 0..8 hold every activation as the
// (hi, lo) bf16 PAIR the next layer consumed (per 8 features 16 B of hi parts, then 16 B of lo parts, in the 1 KB an fp32 row takes),
// slot 9 the fp32 dir_encoding outputs in columns [0, 128) and the ReLU SIGN WORDS of layers 1..8 in its unused half, emb the fp32
// embedded inputs.  Only the SN_DTYPE_BF16X3 forms of sn_mlp_backward_chain / sn_weight_grads read it; handing it to an SN_DTYPE_F32
// entry point (or an fp32 state to these) gives wrong gradients without an error (include/sinnerf_hip.h "pairing rule").
// Row-coalesced stores through per-wave staging tiles, four 1 KB row-group stores per finished tile dealt one per
// k-step behind the slab's DMA pieces; the sync points wait with a COUNTED vmcnt (the four youngest operations of a wave are those
// stores) at a fence-less barrier, and the staging writes are inline asm -- the three measures sn_mlp_bf16.h documents for the
// bf16-state kernels; at this kernel's slab time (48 MFMAs x 32 cycles) a store drain per slab would cost more than the slab.
// Compiler-scheduled C++ around inline-asm MFMAs / epilogue blocks (the register-file discipline of sn_mlp_fwd_bf16.hip:
// hand-managed AGPRs, VGPR accumulators, tools/check_agpr.py on the build).
#include "sn_mlp_x3.h"

namespace snk {

template <bool SIGMA_ONLY, int INPUT_MODE, bool STORE>
__global__ void __launch_bounds__(256)
mlp_fwd_bf16x3_kernel(const char* __restrict__ blob, const float* __restrict__ in0, const float* __restrict__ in1,
                      long P, int S, float* __restrict__ out, float* __restrict__ acts, float* __restrict__ emb, long slot_rows) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds_bias = reinterpret_cast<float*>(smem);
  const float* lds_aux = lds_bias + snl::BIAS_FLOATS;
  asm volatile("" ::: "a0", "a255");             // size the kernel for the whole hand-managed AGPR file

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int j = lane & 31;
  const int h = lane >> 5;
  constexpr int TILE_PTS = 4 * 32;                           // 128 points per workgroup pass
  const long n_tiles = (P + TILE_PTS - 1) / TILE_PTS;
  const long my_tiles = (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x;

  Ring ring;
  ring.blob = blob;
  ring.gnext = blob;
  ring.base = smem + TAIL_LDS_BYTES;
  ring.n_used = SIGMA_ONLY ? snl::SLAB_FIN : snl::N_SLABS;
  ring.stage_id = 0;
  ring.stage_slot = 0;
  ring.remaining = my_tiles * ring.n_used;
  ring.tid = tid;
  ring.wbase = __builtin_amdgcn_readfirstlane((tid & ~63) * 16);
  ring.pieces = 0; ring.piece = 0; ring.slab_bytes = 0;
  ring.stage_whole();
  ring.stage_whole();
  {
    const float4* gb = reinterpret_cast<const float4*>(blob + snl::bias_byte_offset(snl::DT_BF16X3));
    float4* lb = reinterpret_cast<float4*>(lds_bias);
    for (int i = tid; i < snl::TAIL_FLOATS / 4; i += 256) lb[i] = gb[i];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int cslot = 0;
  u32x4 af[4][2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    af[i][0] = *reinterpret_cast<const u32x4*>(ring.slot(0) + lane * 16 + i * 2048);
    af[i][1] = *reinterpret_cast<const u32x4*>(ring.slot(0) + lane * 16 + i * 2048 + 1024);
  }
  f32x16 a0, b0, a1, b1;                                     // chains (A, B) of the two accumulator sets
  a0 = load_bias(lds_bias, 0, h);
  const int n_used = ring.n_used;
  // training forward: per-wave staging tile of the activation stores (sn_mlp_pipe.h XPOSE_*)
  const char* const xp = smem + X3_LDS_BYTES + wave * XPOSE_WAVE_BYTES;
  const unsigned xp_w_lds = (unsigned)(X3_LDS_BYTES + wave * XPOSE_WAVE_BYTES) + (unsigned)(j * XPOSE_PITCH + 4 * h) * 4u;
  const unsigned xp_s_lds = xp_w_lds - 8u * (unsigned)h;           // ... of the split-state tiles: 8 B of hi parts per lane, lo parts 16 B on
  const unsigned xp_r = (unsigned)((lane >> 3) * XPOSE_PITCH + 4 * (lane & 7)) * 4u;    // row lane>>3, 16-byte chunk lane&7
  const unsigned g_off = (unsigned)((lane >> 3) * 256 + 4 * (lane & 7)) * 4u;

  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int ht = h;
    asm volatile("" : "+v"(ht));               // per-tile opaque copy of the lane half (keeps the embedding's selects in the loop)
    const long p_wave = (tile * 4 + __builtin_amdgcn_readfirstlane(wave)) * 32;          // wave-uniform
    const long p_raw = p_wave + j;
    const bool valid = p_raw < P;
    const long p = valid ? p_raw : P - 1;
    u32x4 xh[4], xl[4];                                      // embedded xyz, (hi, lo) operands of the 4 k-steps
    {
      float f[32];
      if (INPUT_MODE == 0) {
        const float* rp = in0 + (p / S) * 8;
        const float zz = in1[p];
        const float x = __fadd_rn(rp[0], __fmul_rn(rp[3], zz));      // xyz = o + d*z, separate roundings (rendering.py:284-285)
        const float y = __fadd_rn(rp[1], __fmul_rn(rp[4], zz));
        const float z = __fadd_rn(rp[2], __fmul_rn(rp[5], zz));
        embed_xyz(x, y, z, ht, f);                                   // the exact embedding of the fp32 kernel
      } else {
        const float* row = in0 + p * (long)S;
        int hh = h;
        asm volatile("" : "+v"(hh));
#pragma unroll
        for (int e = 0; e < 32; ++e) {
          const int c0 = snl::xyz_slot_col(0, e), c1 = snl::xyz_slot_col(1, e);
          const int c = hh ? c1 : c0;
          f[e] = (c >= 0) ? row[c < 0 ? 0 : c] : 0.0f;
        }
      }
      if (STORE && INPUT_MODE == 0) store_emb_xyz(emb + p_raw * 128, f, ht);   // whole 128-point tiles are allocated: no predicate
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        x3_split8(f + 8 * ks, xh[ks], xl[ks]);
        asm volatile("" : "+v"(xh[ks]), "+v"(xl[ks]));
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    int s = 0;
    float sg = 0.0f;                                         // sigma head partial (fp32, this lane half)
    int cur_slot = 0;
    // training forward: the four fp32 values of accumulator registers 4qq..4qq+3 go to the wave's staging tile; store_rows(i) writes
    // row group i (8 points x 128 B) of the staged 32-point x 32-feature tile to acts[slot][point][32t..32t+31], non-temporal
    auto stage = [&](int qq, const float (&v)[4]) __attribute__((always_inline)) {           // fp32 tile (slot 9)
      if (STORE) x3_lds_write_b128(xp_w_lds, 32 * qq, v);
    };
    // slots 0..8: the (hi, lo) pairs the epilogue has just built for the next layer ARE the stored state (sn_layout.h "x3 state")
    auto stage_split = [&](int qq, uint32_t h0, uint32_t h1, uint32_t l0, uint32_t l1) __attribute__((always_inline)) {
      if (STORE) x3_lds_write_split(xp_s_lds, 32 * qq, h0, h1, l0, l1);
    };
    f32x4 rowbuf[1];                                         // row groups between their ds_read and their store (x3_store_step)
    auto rows_read = [&](int i) __attribute__((always_inline)) {
      if (STORE) rowbuf[0] = *reinterpret_cast<const f32x4*>(xp + xp_r + 8 * i * XPOSE_PITCH * 4);
    };
    auto rows_write = [&](int slot, int t, int i) __attribute__((always_inline)) {
      if (STORE) {
        const char* base = reinterpret_cast<const char*>(acts) + (((long)slot * slot_rows + p_wave + 8 * i) * 256 + 32 * t) * 4;
        unsigned go = g_off;
        asm volatile("" : "+v"(go));             // opaque per store: no hoisted per-slot address registers
        __builtin_nontemporal_store(rowbuf[0], reinterpret_cast<f32x4*>(const_cast<char*>(base) + go));
      }
    };
    auto store_rows = [&](int slot, int t, int i) __attribute__((always_inline)) { rows_read(i); rows_write(slot, t, i); };
    // Epilogues of output tile t (chains ra + rb) writing activation set W: dword q of the tile = results 2q, 2q+1 -> k-steps
    // 2t (q < 4), 2t+1 of the next layer, hi part and lo part
    // training forward: ReLU sign words for the backward chain (sn_mlp_x3.h x3_sign_bits): one word per lane and tile PAIR, the four
    // words of a layer leave as ONE 16-byte store per lane into the unused half of slot 9 -- for the 32 points a wave owns, layer l
    // sits in rows first point + 4 l + (lane >> 4), bytes [512 + 16 (lane & 15), + 16): 256 B per point and layer
    uint32_t sgn = 0;
    u32x4 sgn4 = {0u, 0u, 0u, 0u};
    uint32_t c01 = 0x00010001u;
    asm volatile("" : "+v"(c01));
    auto sign_pair = [&](int t, int q, uint32_t h0, uint32_t h1) __attribute__((always_inline)) {
      if (STORE) {
        if ((t & 1) == 0 && q == 0) sgn = 0;
        x3_sign_bits(sgn, h0, q + 8 * (t & 1), c01);
        x3_sign_bits(sgn, h1, q + 1 + 8 * (t & 1), c01);
      }
    };
    auto sign_tile_done = [&](int t) __attribute__((always_inline)) {
      if (STORE && (t & 1)) {
        sgn4[t >> 1] = sgn;
        if (t == 7) {
          char* base = reinterpret_cast<char*>(acts) + (((long)9 * slot_rows + p_wave + 4 * cur_slot) * 256 + 128) * 4;
          unsigned so = (unsigned)((lane >> 4) * 1024 + (lane & 15) * 16);
          asm volatile("" : "+v"(so));
          __builtin_nontemporal_store(sgn4, reinterpret_cast<u32x4*>(base + so));
        }
      }
    };
    // (blk = 0..3: the block of accumulator registers 4 blk .. 4 blk + 3, q = 2 blk)
    auto relu_tile = [&](auto wset, int t, const f32x16& ra, const f32x16& rb, int blk) __attribute__((always_inline)) {
      constexpr int W = decltype(wset)::value;
      {
        const int q = 2 * blk;
        const float a[4] = {ra[2 * q], ra[2 * q + 1], ra[2 * q + 2], ra[2 * q + 3]};
        const float b[4] = {rb[2 * q], rb[2 * q + 1], rb[2 * q + 2], rb[2 * q + 3]};
        float v[4];
        uint32_t h0, h1, l0, l1;
        x3_epi<true>(x3_reg(W, 0, 2 * t + (q >> 2)) + (q & 3), x3_reg(W, 1, 2 * t + (q >> 2)) + (q & 3), a, b, v, h0, h1, l0, l1);
        stage_split(q >> 1, h0, h1, l0, l1);
        sign_pair(t, q, h0, h1);
      }
      if (blk == 3) sign_tile_done(t);
    };
    auto relu_sigma_tile = [&](auto wset, int t, const f32x16& ra, const f32x16& rb, int blk) __attribute__((always_inline)) {   // layer 8
      constexpr int W = decltype(wset)::value;
      const f32x4* ws = reinterpret_cast<const f32x4*>(lds_aux + snl::AUX_SIGW + h * 128 + 16 * t);
      {
        const int q = 2 * blk;
        const f32x4 w = ws[q >> 1];
        const float a[4] = {ra[2 * q], ra[2 * q + 1], ra[2 * q + 2], ra[2 * q + 3]};
        const float b[4] = {rb[2 * q], rb[2 * q + 1], rb[2 * q + 2], rb[2 * q + 3]};
        float v[4];
        uint32_t h0, h1, l0, l1;
        x3_epi<true>(x3_reg(W, 0, 2 * t + (q >> 2)) + (q & 3), x3_reg(W, 1, 2 * t + (q >> 2)) + (q & 3), a, b, v, h0, h1, l0, l1);
        sign_pair(t, q, h0, h1);
        sg = __builtin_fmaf(w[0], v[0], sg);                 // sigma head on the fp32 ReLU outputs (nerf.py:136)
        sg = __builtin_fmaf(w[1], v[1], sg);
        sg = __builtin_fmaf(w[2], v[2], sg);
        sg = __builtin_fmaf(w[3], v[3], sg);
        stage_split(q >> 1, h0, h1, l0, l1);
      }
      if (blk == 3) sign_tile_done(t);
    };
    auto copy_tile = [&](auto wset, int t, const f32x16& ra, const f32x16& rb, int blk) __attribute__((always_inline)) {   // xyz_encoding_final
      constexpr int W = decltype(wset)::value;
      {
        const int q = 2 * blk;
        const float a[4] = {ra[2 * q], ra[2 * q + 1], ra[2 * q + 2], ra[2 * q + 3]};
        const float b[4] = {rb[2 * q], rb[2 * q + 1], rb[2 * q + 2], rb[2 * q + 3]};
        float v[4];
        uint32_t h0, h1, l0, l1;
        x3_epi<false>(x3_reg(W, 0, 2 * t + (q >> 2)) + (q & 3), x3_reg(W, 1, 2 * t + (q >> 2)) + (q & 3), a, b, v, h0, h1, l0, l1);
        stage_split(q >> 1, h0, h1, l0, l1);
      }
    };
#define SNX_LW_CUR (ring.slot(cslot) + lane * 16)
#define SNX_LW_NEXT (ring.slot(cslot == 2 ? 0 : cslot + 1) + lane * 16)
#define SNX_SNEXT (s + 1 == n_used ? 0 : s + 1)
#define SNX_ADVANCE() do { ++s; cslot = (cslot == 2) ? 0 : cslot + 1; } while (0)
#define SNX_W(W_) std::integral_constant<int, W_>{}
    // training forward: the youngest four vector-memory operations of a wave at a slab's sync point are the row stores the
    // previous slab posted behind its DMA pieces (tile T-2's; at T = 0 the previous layer's last tile's) -- except at T = 1,
    // whose predecessor posts none
#define SNX_SLAB(T_, NK0_, NK1_, S0_, S1_, GB_, PH_, NB_, BH_, BL_, EPI_, W_)                                              \
  do {                                                                                                                     \
    constexpr int VW_ = (STORE && (T_) != 1) ? 4 : 0;                                                                      \
    if (((T_) & 1) == 0)                                                                                                   \
      slab_x3<NK0_, NK1_, S0_, S1_, GB_, PH_, NB_, VW_>(a0, b0, a1, af, SNX_LW_CUR, BH_, BL_, SNX_LW_NEXT, lds_bias, SNX_SNEXT, h, ring, \
                                                   [&](int blk) __attribute__((always_inline)) { if ((T_) > 0) EPI_(SNX_W(W_), (T_) - 1, a1, b1, blk); }, \
                                                   [&](int ks, int nk, int st0, bool before) __attribute__((always_inline)) {                    \
                                                     if ((T_) > 0 && !before) x3_store_step(ks, nk, st0, rows_read, [&](int i) __attribute__((always_inline)) { rows_write(cur_slot, (T_) - 1, i); }); }); \
    else                                                                                                                   \
      slab_x3<NK0_, NK1_, S0_, S1_, GB_, PH_, NB_, VW_>(a1, b1, a0, af, SNX_LW_CUR, BH_, BL_, SNX_LW_NEXT, lds_bias, SNX_SNEXT, h, ring, \
                                                   [&](int blk) __attribute__((always_inline)) { EPI_(SNX_W(W_), (T_) - 1, a0, b0, blk); }, \
                                                   [&](int ks, int nk, int st0, bool before) __attribute__((always_inline)) {                    \
                                                     if (!before) x3_store_step(ks, nk, st0, rows_read, [&](int i) __attribute__((always_inline)) { rows_write(cur_slot, (T_) - 1, i); }); }); \
    SNX_ADVANCE();                                                                                                         \
  } while (0)
#define SNX_LAYER(NK0_, NK1_, S0_, S1_, GB_, NBA_, NBB_, EPI_, W_)              \
  do {                                                                          \
    SNX_SLAB(0, NK0_, NK1_, S0_, S1_, GB_, 0, NBA_, xh, xl, EPI_, W_);          \
    SNX_SLAB(1, NK0_, NK1_, S0_, S1_, GB_, 0, NBA_, xh, xl, EPI_, W_);          \
    SNX_SLAB(2, NK0_, NK1_, S0_, S1_, GB_, 0, NBA_, xh, xl, EPI_, W_);          \
    SNX_SLAB(3, NK0_, NK1_, S0_, S1_, GB_, 0, NBA_, xh, xl, EPI_, W_);          \
    SNX_SLAB(4, NK0_, NK1_, S0_, S1_, GB_, 0, NBA_, xh, xl, EPI_, W_);          \
    SNX_SLAB(5, NK0_, NK1_, S0_, S1_, GB_, 0, NBA_, xh, xl, EPI_, W_);          \
    SNX_SLAB(6, NK0_, NK1_, S0_, S1_, GB_, 0, NBB_, xh, xl, EPI_, W_);          \
    SNX_SLAB(7, NK0_, NK1_, S0_, S1_, GB_, 0, NBB_, xh, xl, EPI_, W_);          \
    x3_result_fence(a1, b1);                                                        \
    EPI_(SNX_W(W_), 7, a1, b1, 0); EPI_(SNX_W(W_), 7, a1, b1, 1);               \
    EPI_(SNX_W(W_), 7, a1, b1, 2); EPI_(SNX_W(W_), 7, a1, b1, 3);               \
    store_rows(cur_slot, 7, 0); store_rows(cur_slot, 7, 1);                     \
    store_rows(cur_slot, 7, 2); store_rows(cur_slot, 7, 3);                     \
  } while (0)
    // bytes of the slab kinds (K * 128): the NB_ argument is the slab TWO ahead in the stream
    constexpr int B_L0 = 64 * 128, B_H = 256 * 128, B_SKIP = 320 * 128, B_DIR = 288 * 128;

    // ---- layer 0: reads the xyz embedding (VGPRs), writes set 0
    cur_slot = 0;
    SNX_LAYER(4, 0, -1, -1, 1, B_L0, B_H, relu_tile, 0);
    // ---- layers 1..7: odd layers read set 0 / write set 1, even layers the reverse; skip concat at layer 4 (xyz FIRST,
    //      nerf.py:133); layer 7's epilogues also feed the sigma head
#pragma unroll 1
    for (int l = 1; l < 8; ++l) {
      cur_slot = l;
      if (l == 4) {
        SNX_LAYER(4, 16, -1, 1, 2, B_SKIP, B_H, relu_tile, 0);
      } else if (l == 7) {
        if (SIGMA_ONLY) SNX_LAYER(16, 0, 0, 0, 2, B_H, B_L0, relu_sigma_tile, 1);
        else SNX_LAYER(16, 0, 0, 0, 2, B_H, B_H, relu_sigma_tile, 1);
      } else if (l == 3) {
        SNX_LAYER(16, 0, 0, 0, 2, B_H, B_SKIP, relu_tile, 1);
      } else if (l & 1) {
        SNX_LAYER(16, 0, 0, 0, 2, B_H, B_H, relu_tile, 1);
      } else {
        SNX_LAYER(16, 0, 1, 1, 2, B_H, B_H, relu_tile, 0);
      }
    }
    const float sigma = sg + __shfl_xor(sg, 32, 64) + lds_aux[snl::AUX_HEADB];
    if (SIGMA_ONLY) {
      if (valid && h == 0) out[p_raw] = sigma;
      continue;
    }
    // ---- xyz_encoding_final (no activation): reads set 1, writes set 0
    cur_slot = 8;
    SNX_LAYER(16, 0, 1, 1, 2, B_H, B_DIR, copy_tile, 0);

    // ---- dir_encoding + ShiftedSoftplus: reads set 0 and the dir embedding (VGPRs); rgb head from the fp32 softplus outputs
    u32x4 dh[2], dl[2];
    {
      float f[16];
      if (INPUT_MODE == 0) {
        const float* rp = in0 + (p / S) * 8;
        embed_dir(rp[3], rp[4], rp[5], ht, f);
      } else {
        const float* row = in0 + p * (long)S;
        int hh = h;
        asm volatile("" : "+v"(hh));
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int c0 = snl::dir_slot_col(0, e), c1 = snl::dir_slot_col(1, e);
          const int c = hh ? c1 : c0;
          f[e] = (c >= 0) ? row[63 + (c < 0 ? 0 : c)] : 0.0f;
        }
      }
      if (STORE && INPUT_MODE == 0) store_emb_dir(emb + p_raw * 128 + 64, f, ht);      // columns [64, 91)
      x3_split8(f, dh[0], dl[0]);
      x3_split8(f + 8, dh[1], dl[1]);
      asm volatile("" : "+v"(dh[0]), "+v"(dh[1]), "+v"(dl[0]), "+v"(dl[1]));
      __builtin_amdgcn_sched_barrier(0);
    }
    f32x2 c3[3];
    c3[0] = c3[1] = c3[2] = f32x2{0.0f, 0.0f};
    auto ssp_tile = [&](auto, int t, const f32x16& ra, const f32x16& rb, int q) __attribute__((always_inline)) {
      {
        f32x4 w[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
          w[c] = *reinterpret_cast<const f32x4*>(lds_aux + snl::AUX_RGBW + c * 128 + h * 64 + 16 * t + 4 * q);
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = ra[4 * q + i] + rb[4 * q + i];
        asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(c3[0]), "+v"(c3[1]), "+v"(c3[2]));
        float v[4];
        ssp4_rgb(x, w, c3, v);
        stage(q, v);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // 18 k-steps per slab: the fragment-ring phase alternates 0, 2, 0, 2; tiles 2, 3 stage the next point tile's first slabs
    cur_slot = 9;
    SNX_SLAB(0, 16, 2, 0, -1, 2, 0, B_DIR, dh, dl, ssp_tile, 0);
    SNX_SLAB(1, 16, 2, 0, -1, 2, 2, B_DIR, dh, dl, ssp_tile, 0);
    SNX_SLAB(2, 16, 2, 0, -1, 2, 0, B_L0, dh, dl, ssp_tile, 0);
    SNX_SLAB(3, 16, 2, 0, -1, 2, 2, B_L0, dh, dl, ssp_tile, 0);
    x3_result_fence(a1, b1);
    ssp_tile(SNX_W(0), 3, a1, b1, 0); ssp_tile(SNX_W(0), 3, a1, b1, 1);
    ssp_tile(SNX_W(0), 3, a1, b1, 2); ssp_tile(SNX_W(0), 3, a1, b1, 3);
    store_rows(9, 3, 0); store_rows(9, 3, 1); store_rows(9, 3, 2); store_rows(9, 3, 3);
    {
      float o3[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o3[c] = rgb_activation(hsum(c3[c]) + __shfl_xor(hsum(c3[c]), 32, 64) + lds_aux[snl::AUX_HEADB + 1 + c]);
      if (valid && h == 0) {
        float4 o;
        o.x = o3[0]; o.y = o3[1]; o.z = o3[2]; o.w = sigma;
        reinterpret_cast<float4*>(out)[p_raw] = o;
      }
    }
#undef SNX_LW_CUR
#undef SNX_LW_NEXT
#undef SNX_SNEXT
#undef SNX_ADVANCE
#undef SNX_SLAB
#undef SNX_LAYER
#undef SNX_W
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace snk

extern "C" int SN_LAUNCH_NAME(sn_mlp_forward_bf16x3)(const void* blob, const float* in0, const float* in1, long n_points, int s_or_ld,
                                            int sigma_only, int input_mode, float* out, float* acts, float* emb, long slot_rows,
                                            hipStream_t stream) {
  using namespace snk;
  if (n_points <= 0) return 0;
  const long tiles = (n_points + 127) / 128;
  const bool store = acts != nullptr;
  if (store && (sigma_only || emb == nullptr || slot_rows < tiles * 128)) return SN_E_BADARG;
  dim3 grid(snh::persistent_grid(tiles)), block(256);
  const char* b = reinterpret_cast<const char*>(blob);
  const size_t lds = X3_LDS_BYTES + (store ? XPOSE_LDS_BYTES : 0);
#define SN_LAUNCH(SO, IM, ST)                                                                                        \
  do {                                                                                                               \
    auto kfn = mlp_fwd_bf16x3_kernel<SO, IM, ST>;                                                                    \
    SN_ENSURE_DYN_LDS(kfn, lds);                                                                                     \
    hipLaunchKernelGGL(kfn, grid, block, lds, stream, b, in0, in1, n_points, s_or_ld, out, acts, emb, slot_rows);    \
  } while (0)
  if (store) { if (input_mode == 0) SN_LAUNCH(false, 0, true); else SN_LAUNCH(false, 1, true); }
#ifdef SN_CLASSIC_HEADS                         // the sigma-only kernels never reach the heads: sn_api.hip routes them to the main pass
  else if (sigma_only) return SN_E_UNSUPPORTED;
  else if (input_mode == 0) SN_LAUNCH(false, 0, false);
  else SN_LAUNCH(false, 1, false);
#else
  else if (input_mode == 0) { if (sigma_only) SN_LAUNCH(true, 0, false); else SN_LAUNCH(false, 0, false); }
  else { if (sigma_only) SN_LAUNCH(true, 1, false); else SN_LAUNCH(false, 1, false); }
#endif
#undef SN_LAUNCH
  return (int)hipGetLastError();
}
