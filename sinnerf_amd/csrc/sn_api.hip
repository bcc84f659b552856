// sn_api.hip -- the extern "C" boundary declared in include/sinnerf_hip.h + the weight packer.
#include <hip/hip_fp16.h>
#include "../../include/sinnerf_hip.h"
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_layout.h"

namespace {
struct RawPtrs { const float* p[snl::N_RAW]; };

__device__ __forceinline__ unsigned short f32_to_bf16_rne(float f) {
  unsigned int u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

__global__ void __launch_bounds__(256)
pack_kernel(RawPtrs raw, const snl::PackEntry* __restrict__ table, long n, char* __restrict__ blob, int dtype) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const snl::PackEntry e = table[i];
    float v = 0.0f;
    const bool as_f32 = (e.src == -2) || (e.src >= 0 && (e.src & snl::SRC_F32_FLAG));
    if (e.src >= 0) {
      const int t = (e.src >> 20) & 0x1ff, off = e.src & 0xfffff;
      const float* src = raw.p[0];
#pragma unroll
      for (int k = 1; k < snl::N_RAW; ++k) src = (t == k) ? raw.p[k] : src;
      v = src[off];
    }
    if (dtype == snl::DT_F32 || as_f32) *reinterpret_cast<float*>(blob + e.dst) = v;
    else if (e.src >= 0 && (e.src & snl::SRC_LO_FLAG))             // bf16x3: the remainder of the RNE high part, itself RNE
      *reinterpret_cast<unsigned short*>(blob + e.dst) = f32_to_bf16_rne(__fsub_rn(v, __uint_as_float((unsigned)f32_to_bf16_rne(v) << 16)));
    else if (dtype == snl::DT_F16) *reinterpret_cast<__half*>(blob + e.dst) = __float2half_rn(v);    // SN_DTYPE_F16: fp16 operands (RNE)
    else *reinterpret_cast<unsigned short*>(blob + e.dst) = f32_to_bf16_rne(v);
  }
}

// ---- the `dtype` argument: a base code with flag bits OR-ed in.  Every entry names the bits and the bases it accepts; a bit it does
// not accept stays in the base code and is refused with it.
constexpr unsigned bit(int base) { return 1u << base; }
constexpr unsigned PACKABLE = bit(SN_DTYPE_F32) | bit(SN_DTYPE_BF16) | bit(SN_DTYPE_BF16X3) | bit(SN_DTYPE_F16);       // = the inference set
constexpr unsigned TRAINABLE = bit(SN_DTYPE_F32) | bit(SN_DTYPE_BF16) | bit(SN_DTYPE_BF16_STATE) | bit(SN_DTYPE_BF16X3);
struct Dtype { int base, bits; };
bool parse_dtype(int dtype, int accepted_bits, unsigned accepted_bases, Dtype* d) {
  d->bits = dtype & accepted_bits;
  d->base = dtype & ~accepted_bits;
  return d->base >= 0 && d->base < 32 && (accepted_bases >> d->base & 1u);
}
// points per tile of the MLP kernels of an arithmetic: the training state is stored / written in whole tiles
constexpr long tile_rows(int base) { return (base == SN_DTYPE_F32 || base == SN_DTYPE_BF16X3) ? 128 : 256; }
bool holds_whole_tiles(long slot_rows, long n_points, int base) {
  const long tile = tile_rows(base);
  return slot_rows >= (n_points + tile - 1) / tile * tile;
}
// the state of the weight-gradient entries is read in whole 16-row steps
bool bad_slot_rows(long slot_rows) { return slot_rows < 16 || slot_rows % 16 != 0; }
// the layout sn_mlp_backward_chain(base) left g_acts in for the ray / point gradients: 0 = fp32 rows, 1 = bf16 rows, 2 = x3 state
int g_acts_layout(int base) { return base == SN_DTYPE_BF16_STATE ? 1 : base == SN_DTYPE_BF16X3 ? 2 : 0; }
// a (patch_w, patch_h) window of strides (stride_x, stride_y) at (x0, y0) in an H x W frame, possibly empty: the part of its check
// that is SN_E_BADARG, and the part that is SN_E_BADSHAPE (the window leaves the frame)
bool window_badarg(int H, int W, int stride_x, int stride_y, int patch_w, int patch_h) {
  return H < 1 || W < 1 || stride_x < 1 || stride_y < 1 || patch_w < 0 || patch_h < 0;
}
bool window_badshape(int H, int W, int x0, int y0, int stride_x, int stride_y, int patch_w, int patch_h) {
  return x0 < 0 || y0 < 0 || (patch_w > 0 && x0 + (patch_w - 1) * stride_x >= W) || (patch_h > 0 && y0 + (patch_h - 1) * stride_y >= H);
}
bool packable(int dtype) { Dtype d; return parse_dtype(dtype, 0, PACKABLE, &d); }
// sn_weight_grads and its two queries: SN_DTYPE_EMB_BF16 is the only bit, refused where the kernels cannot read that form (sn_launch.h)
int parse_dw_dtype(int dtype, Dtype* d) {
  if (!parse_dtype(dtype, SN_DTYPE_EMB_BF16, TRAINABLE, d)) return SN_E_UNSUPPORTED;
  d->bits = d->bits ? 1 : 0;                     // = the emb16 argument of the *_impl / *_launch functions
  return snh::emb16_refused(d->base, d->bits) ? SN_E_UNSUPPORTED : 0;
}

// ---- which kernel runs: a pure function of the arguments (no HIP call), exported as sn_mlp_route for the CPU routing test.
// The two compilation passes of the MLP kernels (sn_device.h): SN_DTYPE_CLASSIC_HEADS in `dtype` selects the ReLU / Sigmoid pass; a
// sigma-only evaluation never reaches the heads and always runs the main pass.
#define SN_HEADS(classic, name) ((classic) ? name##_classic_launch : name##_launch)
#define SN_MLP_LAUNCHERS(X)                                                                                                          \
  X(sn_mlp_forward_f32) X(sn_mlp_forward_f32g) X(sn_mlp_forward_f32g_store) X(sn_mlp_forward_bf16) X(sn_mlp_forward_bf16_f16)        \
  X(sn_mlp_forward_bf16_v3) X(sn_mlp_forward_bf16_v3_f16) X(sn_mlp_forward_bf16_t) X(sn_mlp_forward_bf16x3) X(sn_mlp_forward_bf16x3_t) \
  X(sn_mlp_backward_chain_f32) X(sn_mlp_backward_chain_f32g) X(sn_mlp_backward_chain_bf16) X(sn_mlp_backward_chain_bf16_t)           \
  X(sn_mlp_backward_chain_bf16x3) X(sn_mlp_backward_chain_bf16x3_t)
#define SN_X(name) K_##name,
enum Launcher { SN_MLP_LAUNCHERS(SN_X) K_NONE };
#undef SN_X
#define SN_X(name) {#name, #name "_classic"},
const char* const LAUNCHER_NAMES[][2] = {SN_MLP_LAUNCHERS(SN_X)};
#undef SN_X
struct Route { Launcher k; bool classic; };

enum Family { FORWARD, TRAIN, CHAIN };
struct Entry { Family family; int input_mode, dtype_bits; unsigned bases; };
constexpr Entry ENTRIES[] = {
    /* SN_ROUTE_FORWARD          */ {FORWARD, 0, SN_DTYPE_CLASSIC_HEADS, PACKABLE},
    /* SN_ROUTE_FORWARD_EMBEDDED */ {FORWARD, 1, SN_DTYPE_CLASSIC_HEADS, PACKABLE},
    /* SN_ROUTE_TRAIN            */ {TRAIN, 0, SN_DTYPE_CLASSIC_HEADS | SN_DTYPE_COMPILER_SCHEDULED | SN_DTYPE_EMB_BF16, TRAINABLE},
    // (mixed precision keeps bf16 state: no SN_DTYPE_BF16; no previous-generation bit)
    /* SN_ROUTE_TRAIN_EMBEDDED   */ {TRAIN, 1, SN_DTYPE_CLASSIC_HEADS, TRAINABLE & ~bit(SN_DTYPE_BF16)},
    /* SN_ROUTE_CHAIN            */ {CHAIN, 0, SN_DTYPE_CLASSIC_HEADS | SN_DTYPE_COMPILER_SCHEDULED, TRAINABLE},
};
bool accepts(int entry, int dtype, Dtype* d) { return parse_dtype(dtype, ENTRIES[entry].dtype_bits, ENTRIES[entry].bases, d); }
constexpr int FORWARD_FLAGS = SN_FLAG_BF16_COMPILER_SCHEDULED | SN_FLAG_F32_LDS_RING;      // the `flags` bits of the inference entries

// base: an accepted base code; bits: the dtype's flag bits | the SN_FLAG_* bits of `flags` (disjoint values).  K_NONE = refused.
Route route(Family family, int base, int bits, int sigma_only, int input_mode, long n_points) {
  const bool previous = bits & SN_DTYPE_COMPILER_SCHEDULED;
  if (family == FORWARD) {
    const bool classic = (bits & SN_DTYPE_CLASSIC_HEADS) && !sigma_only;
    // the hand-scheduled bf16 / fp16 kernel takes (rays, z_vals) and has no sigma-only form
    const bool hand = input_mode == 0 && !sigma_only && !(bits & SN_FLAG_BF16_COMPILER_SCHEDULED);
    switch (base) {
      case SN_DTYPE_BF16X3: return {K_sn_mlp_forward_bf16x3, classic};     // fp32-level accuracy on the bf16 MFMA: 3-term split
      case SN_DTYPE_F16: return {hand ? K_sn_mlp_forward_bf16_v3_f16 : K_sn_mlp_forward_bf16_f16, classic};    // fp16 operands, bf16 streams
      case SN_DTYPE_BF16: return {hand ? K_sn_mlp_forward_bf16_v3 : K_sn_mlp_forward_bf16, classic};
      // round 6: fragments straight from L2, VALU-free trunk (csrc/sn_mlp_fwd_f32g.hip)
      case SN_DTYPE_F32: return {(bits & SN_FLAG_F32_LDS_RING) ? K_sn_mlp_forward_f32 : K_sn_mlp_forward_f32g, classic};
    }
    return {K_NONE, false};
  }
  const bool classic = bits & SN_DTYPE_CLASSIC_HEADS;
  // the generated instruction streams (sn_mlp_*_t.hip: the same bits as the compiler-scheduled kernels) index points with 32 bits
  const bool generated = !previous && input_mode == 0 && n_points < (1l << 31) - 256;
  Launcher k = K_NONE;
  if (family == TRAIN) {
    switch (base) {
      case SN_DTYPE_BF16X3: k = generated ? K_sn_mlp_forward_bf16x3_t : K_sn_mlp_forward_bf16x3; break;
      case SN_DTYPE_BF16_STATE: k = generated ? K_sn_mlp_forward_bf16_t : K_sn_mlp_forward_bf16; break;
      case SN_DTYPE_BF16: k = K_sn_mlp_forward_bf16; break;
      // round 6: the fragments-from-L2 kernel in store mode (csrc/sn_mlp_fwd_f32g.hip): the same state
      case SN_DTYPE_F32: k = previous ? K_sn_mlp_forward_f32 : K_sn_mlp_forward_f32g_store; break;
    }
    // only the hand-scheduled kernel writes the bf16 form of emb
    if ((bits & SN_DTYPE_EMB_BF16) && k != K_sn_mlp_forward_bf16_t) k = K_NONE;
  } else {
    switch (base) {
      case SN_DTYPE_BF16X3: k = generated ? K_sn_mlp_backward_chain_bf16x3_t : K_sn_mlp_backward_chain_bf16x3; break;
      case SN_DTYPE_BF16_STATE: k = generated ? K_sn_mlp_backward_chain_bf16_t : K_sn_mlp_backward_chain_bf16; break;
      case SN_DTYPE_BF16: k = K_sn_mlp_backward_chain_bf16; break;
      // round 6: the fragments-from-L2 chain (csrc/sn_mlp_bwd_f32g.hip): the same bits
      case SN_DTYPE_F32: k = previous ? K_sn_mlp_backward_chain_f32 : K_sn_mlp_backward_chain_f32g; break;
    }
  }
  return {k, classic};
}

// the forward launchers, inference (acts = emb = nullptr, slot_rows = 0) and training
int launch_forward(Route r, int base, const void* blob, const float* in0, const float* in1, long n_points, int s_or_ld, int sigma_only,
                   int input_mode, float* out, float* acts, float* emb, long slot_rows, int emb16, hipStream_t stream) {
  const int state_bf16 = base == SN_DTYPE_BF16_STATE;
#define SN_FWD(name) return SN_HEADS(r.classic, name)(blob, in0, in1, n_points, s_or_ld, sigma_only, input_mode, out, acts, emb, slot_rows
  switch (r.k) {
    case K_sn_mlp_forward_f32: SN_FWD(sn_mlp_forward_f32), stream);
    case K_sn_mlp_forward_f32g: SN_FWD(sn_mlp_forward_f32g), stream);
    case K_sn_mlp_forward_f32g_store: SN_FWD(sn_mlp_forward_f32g_store), stream);
    case K_sn_mlp_forward_bf16x3: SN_FWD(sn_mlp_forward_bf16x3), stream);
    case K_sn_mlp_forward_bf16: SN_FWD(sn_mlp_forward_bf16), state_bf16, stream);
    case K_sn_mlp_forward_bf16_f16: SN_FWD(sn_mlp_forward_bf16_f16), state_bf16, stream);
#undef SN_FWD
    case K_sn_mlp_forward_bf16_v3: return SN_HEADS(r.classic, sn_mlp_forward_bf16_v3)(blob, in0, in1, n_points, s_or_ld, out, stream);
    case K_sn_mlp_forward_bf16_v3_f16: return SN_HEADS(r.classic, sn_mlp_forward_bf16_v3_f16)(blob, in0, in1, n_points, s_or_ld, out, stream);
    case K_sn_mlp_forward_bf16_t:
      return SN_HEADS(r.classic, sn_mlp_forward_bf16_t)(blob, in0, in1, n_points, s_or_ld, out, acts, emb, slot_rows, emb16, stream);
    case K_sn_mlp_forward_bf16x3_t:
      return SN_HEADS(r.classic, sn_mlp_forward_bf16x3_t)(blob, in0, in1, n_points, s_or_ld, out, acts, emb, slot_rows, stream);
    default: return SN_E_UNSUPPORTED;
  }
}
}  // namespace

extern "C" {

int sn_abi_version(void) { return SN_ABI_VERSION; }

// layout introspection (used by the CPU layout tests; csrc/sn_layout.h is the single source of truth)
int sn_layout_xyz_slot_col(int h, int e) { return (h < 0 || h > 1 || e < 0 || e > 31) ? -2 : snl::xyz_slot_col(h, e); }
int sn_layout_dir_slot_col(int h, int e) { return (h < 0 || h > 1 || e < 0 || e > 15) ? -2 : snl::dir_slot_col(h, e); }
int sn_layout_slab_k(int slab) { return (slab < 0 || slab >= snl::N_SLABS) ? -2 : snl::slab_k(slab); }
int sn_layout_n_slabs(void) { return snl::N_SLABS; }

const char* sn_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case SN_E_BADARG: return "bad argument";
    case SN_E_TOOLARGE: return "problem too large for one launch";
    case SN_E_MISSING_RNG: return "perturb > 0 requires the perturb_rand tensor";
    case SN_E_UNSUPPORTED: return "unsupported configuration (dtype / samples per ray)";
    case SN_E_BADSHAPE: return "bad shape";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

long sn_packed_weights_bytes(int dtype) {
  if (!packable(dtype)) return SN_E_UNSUPPORTED;
  return snl::blob_bytes(dtype);
}
long sn_pack_table_entries(void) { return snl::table_entries(); }
long sn_pack_table_entries_dtype(int dtype) {
  if (!packable(dtype)) return SN_E_UNSUPPORTED;
  return snl::table_entries_dt(dtype);
}

int sn_build_pack_table(int dtype, int32_t* table_host) {
  if (!packable(dtype)) return SN_E_UNSUPPORTED;
  if (!table_host) return SN_E_BADARG;
  snl::build_pack_table(dtype, reinterpret_cast<snl::PackEntry*>(table_host));
  return 0;
}

long sn_packed_weights_bytes_bwd(void) { return snl::bblob_bytes(); }
long sn_pack_table_entries_bwd(void) { return snl::b_table_entries(); }
int sn_build_pack_table_bwd(int32_t* table_host) {
  if (!table_host) return SN_E_BADARG;
  snl::build_pack_table_bwd(reinterpret_cast<snl::PackEntry*>(table_host));
  return 0;
}

long sn_packed_weights_bytes_bwd_bf16(void) { return snl::bbblob_bytes(); }
long sn_pack_table_entries_bwd_bf16(void) { return snl::bb_table_entries(); }
int sn_build_pack_table_bwd_bf16(int32_t* table_host) {
  if (!table_host) return SN_E_BADARG;
  snl::build_pack_table_bwd_bf16(reinterpret_cast<snl::PackEntry*>(table_host));
  return 0;
}

long sn_packed_weights_bytes_bwd_bf16x3(void) { return snl::bbxblob_bytes(); }
long sn_pack_table_entries_bwd_bf16x3(void) { return snl::bbx_table_entries(); }
int sn_build_pack_table_bwd_bf16x3(int32_t* table_host) {
  if (!table_host) return SN_E_BADARG;
  snl::build_pack_table_bwd_bf16x3(reinterpret_cast<snl::PackEntry*>(table_host));
  return 0;
}

int sn_pack_weights(const float* const* raw, const int32_t* table, long n_entries, void* blob, int dtype, void* stream) {
  if (!packable(dtype)) return SN_E_UNSUPPORTED;
  if (!raw || !table || !blob || n_entries <= 0) return SN_E_BADARG;
  RawPtrs rp;
  for (int i = 0; i < snl::N_RAW; ++i) {
    if (!raw[i]) return SN_E_BADARG;
    rp.p[i] = raw[i];
  }
  hipLaunchKernelGGL(pack_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, rp,
                     reinterpret_cast<const snl::PackEntry*>(table), n_entries, reinterpret_cast<char*>(blob), dtype);
  return (int)hipGetLastError();
}

int sn_sample_coarse(const float* rays, long n_rays, int n_samples, int use_disp, float perturb,
                     const float* perturb_rand, float* z_vals, void* stream) {
  if (!rays || !z_vals || n_rays < 0 || n_samples < 1) return SN_E_BADARG;
  return sn_sample_coarse_launch(rays, n_rays, n_samples, use_disp, perturb, perturb_rand, z_vals, (hipStream_t)stream);
}

const char* sn_mlp_route(int entry, int dtype, int flags, int sigma_only, long n_points) {
  if (entry < 0 || entry >= (int)(sizeof(ENTRIES) / sizeof(ENTRIES[0]))) return nullptr;
  const Entry& e = ENTRIES[entry];
  Dtype d;
  if (!accepts(entry, dtype, &d)) return nullptr;
  const bool fwd = e.family == FORWARD;
  const Route r = route(e.family, d.base, d.bits | (fwd ? flags & FORWARD_FLAGS : 0), fwd && sigma_only, e.input_mode, n_points);
  return r.k == K_NONE ? nullptr : LAUNCHER_NAMES[r.k][r.classic];
}

int sn_mlp_forward(const void* blob, int dtype, const float* rays, const float* z_vals, long n_rays, int n_samples,
                   int sigma_only, int flags, float* out, void* stream) {
  if (!blob || !rays || !z_vals || !out || n_rays < 0 || n_samples < 1) return SN_E_BADARG;
  Dtype d;
  if (!accepts(SN_ROUTE_FORWARD, dtype, &d)) return SN_E_UNSUPPORTED;
  return launch_forward(route(FORWARD, d.base, d.bits | (flags & FORWARD_FLAGS), sigma_only, 0, 0), d.base, blob, rays, z_vals,
                        n_rays * (long)n_samples, n_samples, sigma_only, 0, out, nullptr, nullptr, 0, 0, (hipStream_t)stream);
}

int sn_mlp_forward_embedded(const void* blob, int dtype, const float* x, long n_rows, int ld, int sigma_only,
                            int flags, float* out, void* stream) {
  if (!blob || !x || !out || n_rows < 0) return SN_E_BADARG;
  if (ld < (sigma_only ? 63 : 90)) return SN_E_BADSHAPE;
  Dtype d;
  if (!accepts(SN_ROUTE_FORWARD_EMBEDDED, dtype, &d)) return SN_E_UNSUPPORTED;
  return launch_forward(route(FORWARD, d.base, d.bits | (flags & FORWARD_FLAGS), sigma_only, 1, 0), d.base, blob, x, nullptr, n_rows, ld,
                        sigma_only, 1, out, nullptr, nullptr, 0, 0, (hipStream_t)stream);
}

// SN_DTYPE_BF16X3: fp32-level forward on the bf16 MFMA.  Its training state is the "x3 state" of sn_layout.h -- slots 0..8 hold (hi, lo)
// bf16 PAIRS in the bytes of an fp32 row, slot 9 fp32 values + ReLU sign words -- NOT the array SN_DTYPE_F32 writes: only the
// SN_DTYPE_BF16X3 forms of sn_mlp_backward_chain / sn_weight_grads read it (include/sinnerf_hip.h "pairing rule")
int sn_mlp_forward_train(const void* blob, int dtype, const float* rays, const float* z_vals, long n_rays, int n_samples,
                         float* out, float* acts, float* emb, long slot_rows, void* stream) {
  if (!blob || !rays || !z_vals || !out || !acts || !emb || n_rays < 0 || n_samples < 1) return SN_E_BADARG;
  Dtype d;
  if (!accepts(SN_ROUTE_TRAIN, dtype, &d)) return SN_E_UNSUPPORTED;
  const long n_points = n_rays * (long)n_samples;
  if (!holds_whole_tiles(slot_rows, n_points, d.base)) return SN_E_BADSHAPE;
  const Route r = route(TRAIN, d.base, d.bits, 0, 0, n_points);
  if (r.k == K_NONE) return SN_E_UNSUPPORTED;                                  // SN_DTYPE_EMB_BF16 without the kernel that writes it
  if (d.base == SN_DTYPE_BF16X3 && slot_rows % 128 != 0) return SN_E_BADSHAPE;  // whole 128-point tiles, as the header states
  return launch_forward(r, d.base, blob, rays, z_vals, n_points, n_samples, 0, 0, out, acts, emb, slot_rows,
                        (d.bits & SN_DTYPE_EMB_BF16) ? 1 : 0, (hipStream_t)stream);
}

int sn_mlp_forward_train_embedded(const void* blob, int dtype, const float* x, long n_rows, int ld, float* out,
                                  float* acts, long slot_rows, void* stream) {
  if (!blob || !x || !out || !acts || n_rows < 0) return SN_E_BADARG;
  float* emb = acts;                             // not written for pre-embedded rows (the kernels only need it non-null)
  if (ld < 90) return SN_E_BADSHAPE;
  Dtype d;
  if (!accepts(SN_ROUTE_TRAIN_EMBEDDED, dtype, &d)) return SN_E_UNSUPPORTED;
  if (!holds_whole_tiles(slot_rows, n_rows, d.base)) return SN_E_BADSHAPE;
  return launch_forward(route(TRAIN, d.base, d.bits, 0, 1, n_rows), d.base, blob, x, nullptr, n_rows, ld, 0, 1, out, acts, emb, slot_rows, 0,
                        (hipStream_t)stream);
}

// SN_DTYPE_BF16X3 (blob: *_bwd_bf16x3 table): acts MUST be the x3 state sn_mlp_forward_train(SN_DTYPE_BF16X3) wrote (masks from its
// sign words); g_acts leaves in the same layout ((hi, lo) pairs in slots 0..8) for sn_weight_grads(SN_DTYPE_BF16X3)
int sn_mlp_backward_chain(const void* blob_bwd, int dtype, const float* acts, const float* out_raw, const float* g_raw,
                          long n_points, long slot_rows, float* g_acts, float* g_out, void* stream) {
  if (!blob_bwd || !acts || !out_raw || !g_raw || !g_acts || !g_out || n_points < 0) return SN_E_BADARG;
  Dtype d;
  if (!accepts(SN_ROUTE_CHAIN, dtype, &d)) return SN_E_UNSUPPORTED;
  if (!holds_whole_tiles(slot_rows, n_points, d.base)) return SN_E_BADSHAPE;    // whole point tiles are written
  if (d.base == SN_DTYPE_BF16X3 && slot_rows % 128 != 0) return SN_E_BADSHAPE;
  const Route r = route(CHAIN, d.base, d.bits, 0, 0, n_points);
#define SN_CHAIN(name) return SN_HEADS(r.classic, name)(blob_bwd, acts, out_raw, g_raw, n_points, slot_rows, g_acts, g_out
  switch (r.k) {
    case K_sn_mlp_backward_chain_f32: SN_CHAIN(sn_mlp_backward_chain_f32), (hipStream_t)stream);
    case K_sn_mlp_backward_chain_f32g: SN_CHAIN(sn_mlp_backward_chain_f32g), (hipStream_t)stream);
    case K_sn_mlp_backward_chain_bf16: SN_CHAIN(sn_mlp_backward_chain_bf16), d.base == SN_DTYPE_BF16_STATE, (hipStream_t)stream);
    case K_sn_mlp_backward_chain_bf16_t: SN_CHAIN(sn_mlp_backward_chain_bf16_t), (hipStream_t)stream);
    case K_sn_mlp_backward_chain_bf16x3: SN_CHAIN(sn_mlp_backward_chain_bf16x3), (hipStream_t)stream);
    case K_sn_mlp_backward_chain_bf16x3_t: SN_CHAIN(sn_mlp_backward_chain_bf16x3_t), (hipStream_t)stream);
    default: return SN_E_UNSUPPORTED;
  }
#undef SN_CHAIN
}

int sn_generate_rays(const float* c2w, int H, int W, float focal, float near, float far, int x0, int y0, int stride_x,
                     int stride_y, int patch_w, int patch_h, float* rays, void* stream) {
  if (!c2w || !rays || window_badarg(H, W, stride_x, stride_y, patch_w, patch_h)) return SN_E_BADARG;
  if (window_badshape(H, W, x0, y0, stride_x, stride_y, patch_w, patch_h)) return SN_E_BADSHAPE;
  return sn_generate_rays_launch(c2w, H, W, focal, near, far, x0, y0, stride_x, stride_y, patch_w, patch_h, rays,
                                 (hipStream_t)stream);
}

int sn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int step, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return SN_E_BADARG;
  return sn_adam_step_launch(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step,
                             (hipStream_t)stream);
}

// ---- the reference's other optimisers (sn_optim.hip): every refusal below returns before a launch
int sn_sgd_step(float* params, const float* grads, float* momentum_buf, long n, double lr, double momentum, double weight_decay,
                void* stream) {
  if (!params || !grads || n < 0 || (momentum != 0.0 && !momentum_buf)) return SN_E_BADARG;
  return sn_sgd_step_launch(params, grads, momentum_buf, n, lr, momentum, weight_decay, (hipStream_t)stream);
}

int sn_radam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, double beta1, double beta2, double eps,
                  double decay, double step_coeff, int rectified, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n < 0) return SN_E_BADARG;
  return sn_radam_step_launch(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, decay, step_coeff, rectified, nullptr, 0.0, 0,
                              (hipStream_t)stream);
}

int sn_ranger_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, double beta1, double beta2, double eps,
                   double decay, double step_coeff, int rectified, float* slow, double alpha, int sync, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !slow || n < 0 || step_coeff < 0.0) return SN_E_BADARG;
  return sn_radam_step_launch(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, decay, step_coeff, rectified, slow, alpha, sync,
                              (hipStream_t)stream);
}

long sn_render_loss_workspace_bytes(void) { return sn_render_loss_workspace_bytes_impl(); }

int sn_render_loss(const float* rgb_coarse, const float* rgb_fine, const float* depth_coarse, const float* depth_fine,
                   const float* rgb_gt, const float* depth_gt, const unsigned char* mask, int mask_mode, long n,
                   float w_rgb, float w_depth, float* g_rgb_coarse, float* g_rgb_fine, float* g_depth_coarse,
                   float* g_depth_fine, void* workspace, float* out, void* stream) {
  if (!workspace || !out || n < 1 || mask_mode < 0 || mask_mode > 2) return SN_E_BADARG;
  if ((mask_mode == 2 && !mask) || (mask_mode != 0 && !depth_gt)) return SN_E_BADARG;
  if ((rgb_coarse || rgb_fine) && !rgb_gt) return SN_E_BADARG;
  if ((depth_coarse || depth_fine) && !depth_gt) return SN_E_BADARG;
  return sn_render_loss_launch(rgb_coarse, rgb_fine, depth_coarse, depth_fine, rgb_gt, depth_gt, mask, mask_mode, n,
                               w_rgb, w_depth, g_rgb_coarse, g_rgb_fine, g_depth_coarse, g_depth_fine, workspace, out,
                               (hipStream_t)stream);
}

// ---- the losses on the rendered patches (sn_patch_loss.hip): every refusal below returns before a launch
namespace {
// B, H, W, C > 0 and fewer than 2^31 elements: grids, the int tile arithmetic and the workspace offsets stay in range
int check_patch(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return SN_E_BADARG;
  const __int128 n = (__int128)B * H * W * C;
  return n >= ((__int128)1 << 31) ? SN_E_TOOLARGE : 0;
}
}  // namespace

long sn_patch_loss_workspace_bytes(int B, int H, int W, int C, int use_ssim) {
  if (const int refused = check_patch(B, H, W, C)) return refused;
  return sn_patch_loss_workspace_bytes_impl(B, H, W, C, use_ssim ? 1 : 0);
}

int sn_patch_loss(const float* coarse, const float* fine, const float* target, int B, int H, int W, int C, int use_ssim, int window,
                  float w_mse, float w_ssim, float* g_coarse, float* g_fine, void* workspace, float* out, void* stream) {
  if (!target || !workspace || !out || (!coarse && !fine)) return SN_E_BADARG;
  if (const int refused = check_patch(B, H, W, C)) return refused;
  if (use_ssim) {
    if (!fine || window <= 0 || window % 2 == 0 || (C != 1 && C != 3)) return SN_E_BADARG;
    if (H <= window / 2 || W <= window / 2) return SN_E_BADSHAPE;                // reflect padding needs pad < size
    if (window > SN_PATCH_LOSS_MAX_WINDOW) return SN_E_UNSUPPORTED;              // the tile with its halo must fit in LDS
  }
  return sn_patch_loss_launch(coarse, fine, target, B, H, W, C, use_ssim ? 1 : 0, window, w_mse, w_ssim, g_coarse, g_fine, workspace, out,
                              (hipStream_t)stream);
}

long sn_depth_smoothness_workspace_bytes(void) { return sn_depth_smoothness_workspace_bytes_impl(); }

int sn_depth_smoothness(const float* idepth, const float* image, int B, int H, int W, int C, float* g_idepth, float* g_image,
                        void* workspace, float* out, void* stream) {
  if (!idepth || !image || !workspace || !out) return SN_E_BADARG;
  if (const int refused = check_patch(B, H, W, C)) return refused;
  if (H < 2 || W < 2) return SN_E_BADSHAPE;
  return sn_depth_smoothness_launch(idepth, image, B, H, W, C, g_idepth, g_image, workspace, out, (hipStream_t)stream);
}

// ---- the regularisers on a ray's compositing weights (sn_ray_reg.hip)
long sn_ray_regularizers_workspace_bytes(long n_rays) { return sn_ray_regularizers_workspace_bytes_impl(n_rays); }

int sn_ray_regularizers(const float* weights, const float* z_vals, const float* rays, long n_rays, int n_samples, float w_dist,
                        float w_ent, float ent_threshold, float* g_weights, float* per_ray, void* workspace, float* out, void* stream) {
  if (!weights || !z_vals || !rays || !workspace || !out) return SN_E_BADARG;
  if (n_samples < 1 || n_samples > 1024) return SN_E_BADSHAPE;
  return sn_ray_regularizers_launch(weights, z_vals, rays, n_rays, n_samples, w_dist, w_ent, ent_threshold, g_weights, per_ray,
                                    workspace, out, (hipStream_t)stream);
}

// ---- the unseen-view reprojection loss (sn_reproject.hip): every refusal below returns before a launch
long sn_reproject_loss_workspace_bytes(long n) {
  if (n >= (1l << 31)) return SN_E_TOOLARGE;
  return sn_reproject_loss_workspace_bytes_impl(n);
}

int sn_reproject_loss(const float* rays, const float* depth, const float* rgb, const float* opacity, long n, int C,
                      const float* ref_image, const float* ref_depth, int H, int W, const double* ref_proj, float occ_tol,
                      float charb_eps, float z_min, float opacity_threshold, float w_photo, float w_free, float* g_depth, float* g_rgb,
                      float* per_pixel, unsigned char* flags, void* workspace, float* out, void* stream) {
  if (!rays || !depth || !rgb || !ref_image || !ref_depth || !ref_proj || !workspace || !out) return SN_E_BADARG;
  if (H < 2 || W < 2 || C < 1 || C > 4) return SN_E_BADARG;
  if (n >= (1l << 31) || (long)H * W * C >= (1l << 31)) return SN_E_TOOLARGE;
  return sn_reproject_loss_launch(rays, depth, rgb, opacity, n, C, ref_image, ref_depth, H, W, ref_proj, occ_tol, charb_eps, z_min,
                                  opacity_threshold, w_photo, w_free, g_depth, g_rgb, per_pixel, flags, workspace, out,
                                  (hipStream_t)stream);
}

// ---- the unseen-view forward warp (sn_warp.hip): every refusal below returns before a launch
namespace {
int check_frame(int H, int W) {
  if (H <= 0 || W <= 0) return SN_E_BADARG;
  return (long)H * W >= (1l << 31) ? SN_E_TOOLARGE : 0;
}
}  // namespace

long sn_forward_warp_workspace_bytes(int H, int W) {
  if (const int refused = check_frame(H, W)) return refused;
  return sn_forward_warp_workspace_bytes_impl(H, W);
}

int sn_forward_warp(const float* ref_depth, const float* data, int H, int W, int C, const double* ref_proj, const double* src_proj,
                    double eps, int mode, int x0, int y0, int stride_x, int stride_y, int out_w, int out_h, float* out_new,
                    float* new_depth, unsigned char* mask, int* winner, void* workspace, void* stream) {
  if (!ref_depth || !ref_proj || !src_proj || !workspace) return SN_E_BADARG;
  if (const int refused = check_frame(H, W)) return refused;
  if (stride_x <= 0 || stride_y <= 0 || out_w <= 0 || out_h <= 0 || (mode != 0 && mode != 1) || (data && C <= 0)) return SN_E_BADARG;
  if (x0 < 0 || y0 < 0 || x0 + (long)(out_w - 1) * stride_x >= W || y0 + (long)(out_h - 1) * stride_y >= H) return SN_E_BADARG;
  return sn_forward_warp_launch(ref_depth, data, H, W, C, ref_proj, src_proj, eps, mode, x0, y0, stride_x, stride_y, out_w, out_h,
                                out_new, new_depth, mask, winner, workspace, (hipStream_t)stream);
}

long sn_select_landed_workspace_bytes(long n) {
  if (n <= 0) return SN_E_BADARG;
  if (n >= (1l << 31)) return SN_E_TOOLARGE;
  return sn_select_landed_workspace_bytes_impl(n);
}

int sn_select_landed(const unsigned char* mask, long n, const float* u, long m, int* idx, int* n_landed, void* workspace, void* stream) {
  if (!mask || !workspace || n <= 0 || m < 0 || (m > 0 && (!u || !idx))) return SN_E_BADARG;
  if (n >= (1l << 31) || m >= (1l << 31)) return SN_E_TOOLARGE;
  return sn_select_landed_launch(mask, n, u, m, idx, n_landed, workspace, (hipStream_t)stream);
}

namespace {
// a (patch_w, patch_h) window of strides (stride_x, stride_y): how many origins keep it inside the frame, per axis; <= 0: none
long origins_that_fit(int extent, int patch, int stride) { return (long)extent - (long)(patch - 1) * stride; }
}  // namespace

long sn_valid_windows_workspace_bytes(int H, int nx) {
  if (H <= 0 || nx <= 0) return SN_E_BADARG;
  if ((long)H * nx >= (1l << 31)) return SN_E_TOOLARGE;
  return sn_valid_windows_workspace_bytes_impl(H, nx);
}

int sn_valid_windows(const unsigned char* mask, int H, int W, int stride_x, int stride_y, int patch_w, int patch_h, int nx, int ny,
                     unsigned char* valid, int* n_valid, void* workspace, void* stream) {
  if (!mask || !valid || !workspace) return SN_E_BADARG;
  if (const int refused = check_frame(H, W)) return refused;
  if (stride_x <= 0 || stride_y <= 0 || patch_w <= 0 || patch_h <= 0 || nx <= 0 || ny <= 0) return SN_E_BADARG;
  if (nx > origins_that_fit(W, patch_w, stride_x) || ny > origins_that_fit(H, patch_h, stride_y)) return SN_E_BADARG;
  return sn_valid_windows_launch(mask, H, W, stride_x, stride_y, patch_w, patch_h, nx, ny, valid, n_valid, workspace,
                                 (hipStream_t)stream);
}

int sn_gather_windows(const void* const* src, void* const* dst, const int* channels, int n_src, unsigned planar_mask, int H, int W,
                      const int* origin, int stride_x, int stride_y, int patch_w, int patch_h, void* stream) {
  if (!src || !dst || !channels || !origin || n_src <= 0 || n_src > SN_GATHER_MAX_SOURCES) return SN_E_BADARG;
  if (const int refused = check_frame(H, W)) return refused;
  if (stride_x <= 0 || stride_y <= 0 || patch_w <= 0 || patch_h <= 0) return SN_E_BADARG;
  if (origins_that_fit(W, patch_w, stride_x) < 1 || origins_that_fit(H, patch_h, stride_y) < 1) return SN_E_BADARG;
  if (n_src < 32 && (planar_mask >> n_src) != 0) return SN_E_BADARG;
  for (int k = 0; k < n_src; ++k) {
    if (!src[k] || !dst[k] || channels[k] <= 0) return SN_E_BADARG;
    if ((long)H * W * channels[k] >= (1l << 31)) return SN_E_TOOLARGE;
  }
  return sn_gather_windows_launch(src, dst, channels, n_src, planar_mask, H, W, origin, stride_x, stride_y, patch_w, patch_h,
                                  (hipStream_t)stream);
}

int sn_dw_gemm(const void* tasks, int n_tasks, void* stream) {
  if (!tasks || n_tasks < 0) return SN_E_BADARG;
  return sn_dw_launch(tasks, n_tasks, (hipStream_t)stream);
}

long sn_weight_grads_workspace_bytes(long slot_rows, int dtype) {
  if (bad_slot_rows(slot_rows)) return SN_E_BADSHAPE;
  Dtype d;
  if (const int refused = parse_dw_dtype(dtype, &d)) return refused;
  return sn_weight_grads_workspace_bytes_impl(slot_rows, d.base, d.bits);
}

int sn_weight_grads_plan(long slot_rows, int dtype, int32_t* out_host, int max_probs) {
  // the checks of sn_weight_grads_workspace_bytes, in its order
  if (bad_slot_rows(slot_rows)) return SN_E_BADSHAPE;
  Dtype d;
  if (const int refused = parse_dw_dtype(dtype, &d)) return refused;
  if (max_probs < 0 || (max_probs > 0 && !out_host)) return SN_E_BADARG;
  static_assert(sizeof(int32_t) == sizeof(int), "plan records are int32");
  return sn_weight_grads_plan_impl(slot_rows, d.base, d.bits, reinterpret_cast<int*>(out_host), max_probs);
}

int sn_weight_grads(const void* acts, const float* emb, const void* g_acts, long slot_rows, int dtype, void* workspace,
                    float* const* grads, int accumulate, void* stream) {
  if (!acts || !emb || !g_acts || !workspace || !grads) return SN_E_BADARG;
  if (bad_slot_rows(slot_rows)) return SN_E_BADSHAPE;
  Dtype d;
  if (const int refused = parse_dw_dtype(dtype, &d)) return refused;
  return sn_weight_grads_launch(acts, emb, g_acts, slot_rows, d.base, d.bits, workspace, grads, accumulate ? 1 : 0, (hipStream_t)stream);
}

int sn_composite_backward(const float* raw, const float* z_vals, const float* rays, const float* noise, float noise_std,
                          long n_rays, int n_samples, int white_back, const float* g_rgb, const float* g_depth,
                          const float* g_weights, float* g_raw, void* stream) {
  if (!raw || !z_vals || !rays || !g_raw || n_rays < 0 || n_samples < 1) return SN_E_BADARG;
  return sn_composite_backward_launch(raw, z_vals, rays, noise, noise_std, n_rays, n_samples, white_back, g_rgb, g_depth,
                                      g_weights, g_raw, (hipStream_t)stream);
}

int sn_composite_backward_rays(const float* raw, const float* z_vals, const float* rays, const float* noise, float noise_std,
                               long n_rays, int n_samples, int white_back, const float* g_rgb, const float* g_depth,
                               const float* g_weights, float* g_raw, float* g_rays, void* stream) {
  if (!raw || !z_vals || !rays || !g_raw || !g_rays || n_rays < 0 || n_samples < 1) return SN_E_BADARG;
  return sn_composite_backward_rays_launch(raw, z_vals, rays, noise, noise_std, n_rays, n_samples, white_back, g_rgb, g_depth,
                                           g_weights, g_raw, g_rays, (hipStream_t)stream);
}

long sn_ray_grads_workspace_bytes(long n_rays, int n_samples) {
  if (n_rays < 0 || n_samples < 1 || n_samples > 1024) return SN_E_BADSHAPE;
  return sn_ray_grads_workspace_bytes_impl(n_rays, n_samples);
}

int sn_ray_grads(const float* w1, const float* w5, const float* wdir, int dtype, const void* g_acts, long slot_rows,
                 const float* rays, const float* z_vals, long n_rays, int n_samples, void* workspace, float* g_rays,
                 void* stream) {
  if (!w1 || !w5 || !wdir || !g_acts || !rays || !z_vals || !workspace || !g_rays || n_rays < 0) return SN_E_BADARG;
  if (n_samples < 1 || n_samples > 1024) return SN_E_BADSHAPE;
  if (slot_rows < n_rays * (long)n_samples) return SN_E_BADSHAPE;
  // the layout sn_mlp_backward_chain(dtype) left g_acts in; no flag bits: the heads and the kernel generation do not change it
  Dtype d;
  if (!parse_dtype(dtype, 0, TRAINABLE, &d)) return SN_E_UNSUPPORTED;
  return sn_ray_grads_launch(w1, w5, wdir, g_acts_layout(d.base), g_acts, slot_rows, rays, z_vals, n_rays, n_samples, workspace, g_rays,
                             (hipStream_t)stream);
}

int sn_point_grads(const float* w1, const float* w5, int dtype, const void* g_acts, long slot_rows, const float* rays,
                   const float* z_vals, long n_rays, int n_samples, float* g_xyz, void* stream) {
  if (!w1 || !w5 || !g_acts || !rays || !z_vals || !g_xyz) return SN_E_BADARG;
  if (n_samples < 1 || n_samples > 1024) return SN_E_BADSHAPE;
  if (n_rays > 0 && slot_rows < n_rays * (long)n_samples) return SN_E_BADSHAPE;
  // the layout sn_mlp_backward_chain(dtype) left g_acts in, as for sn_ray_grads: no flag bits
  Dtype d;
  if (!parse_dtype(dtype, 0, TRAINABLE, &d)) return SN_E_UNSUPPORTED;
  return sn_point_grads_launch(w1, w5, g_acts_layout(d.base), g_acts, slot_rows, rays, z_vals, n_rays, n_samples, g_xyz, (hipStream_t)stream);
}

int sn_point_grads_wsum(const float* g_xyz, const float* weights, long n_rays, int n_samples, float* g_sum, void* stream) {
  if (!g_xyz || !weights || !g_sum) return SN_E_BADARG;
  if (n_samples < 1 || n_samples > 1024) return SN_E_BADSHAPE;
  return sn_point_grads_wsum_launch(g_xyz, weights, n_rays, n_samples, g_sum, (hipStream_t)stream);
}

long sn_generate_rays_backward_workspace_bytes(void) { return sn_generate_rays_backward_workspace_bytes_impl(); }

int sn_generate_rays_backward(const float* g_rays, int H, int W, float focal, int x0, int y0, int stride_x, int stride_y,
                              int patch_w, int patch_h, void* workspace, float* g_c2w, void* stream) {
  if (!g_rays || !workspace || !g_c2w || window_badarg(H, W, stride_x, stride_y, patch_w, patch_h)) return SN_E_BADARG;
  if (window_badshape(H, W, x0, y0, stride_x, stride_y, patch_w, patch_h)) return SN_E_BADSHAPE;
  return sn_generate_rays_backward_launch(g_rays, H, W, focal, x0, y0, stride_x, stride_y, patch_w, patch_h, workspace, g_c2w,
                                          (hipStream_t)stream);
}

// ---- cameras (fx, fy, cx, cy, sign convention) and the NDC map
namespace {
bool positive_finite(float v) { return v > 0.0f && v <= 3.402823466e38f; }                     // false for NaN and +inf
// -1./(W/(2.*focal)), -1./(H/(2.*focal)) as Python forms them (datasets/ray_utils.py:153-158): in double, cast to fp32 once
float ndc_scale(int size, float focal) { return (float)(-1.0 / ((double)size / (2.0 * (double)focal))); }

int check_camera(int H, int W, float fx, float fy, int convention, int ndc, float ndc_focal, int x0, int y0, int stride_x, int stride_y,
                 int patch_w, int patch_h) {
  if (window_badarg(H, W, stride_x, stride_y, patch_w, patch_h)) return SN_E_BADARG;
  if ((convention != 0 && convention != 1) || (ndc != 0 && ndc != 1)) return SN_E_BADARG;
  if (!positive_finite(fx) || !positive_finite(fy) || !positive_finite(ndc_focal)) return SN_E_BADARG;
  if (window_badshape(H, W, x0, y0, stride_x, stride_y, patch_w, patch_h)) return SN_E_BADSHAPE;
  return 0;
}
}  // namespace

int sn_generate_rays_cam(const float* c2w, int H, int W, float fx, float fy, float cx, float cy, int convention, int ndc,
                         float ndc_focal, float ndc_near, float near, float far, int x0, int y0, int stride_x, int stride_y,
                         int patch_w, int patch_h, float* rays, void* stream) {
  if (!c2w || !rays) return SN_E_BADARG;
  if (const int refused = check_camera(H, W, fx, fy, convention, ndc, ndc_focal, x0, y0, stride_x, stride_y, patch_w, patch_h))
    return refused;
  return sn_generate_rays_cam_launch(c2w, fx, fy, cx, cy, convention, ndc, ndc_scale(W, ndc_focal), ndc_scale(H, ndc_focal), ndc_near,
                                     near, far, x0, y0, stride_x, stride_y, patch_w, patch_h, rays, nullptr, H, W, (hipStream_t)stream);
}

int sn_generate_rays_cam_backward(const float* g_rays, const float* c2w, int H, int W, float fx, float fy, float cx, float cy,
                                  int convention, int ndc, float ndc_focal, float ndc_near, int x0, int y0, int stride_x,
                                  int stride_y, int patch_w, int patch_h, void* workspace, float* g_c2w, void* stream) {
  if (!g_rays || !workspace || !g_c2w) return SN_E_BADARG;
  if (const int refused = check_camera(H, W, fx, fy, convention, ndc, ndc_focal, x0, y0, stride_x, stride_y, patch_w, patch_h))
    return refused;
  if (ndc && !c2w) return SN_E_BADARG;            // the NDC adjoint is taken at the world ray, which comes from c2w
  return sn_generate_rays_cam_backward_launch(g_rays, c2w, fx, fy, cx, cy, convention, ndc, ndc_scale(W, ndc_focal),
                                              ndc_scale(H, ndc_focal), ndc_near, x0, y0, stride_x, stride_y, patch_w, patch_h, workspace,
                                              g_c2w, nullptr, H, W, nullptr, (hipStream_t)stream);
}

int sn_ndc_rays(const float* rays_in, long n_rays, int H, int W, float focal, float ndc_near, float* rays_out, void* stream) {
  if (!rays_in || !rays_out || n_rays < 0 || H < 1 || W < 1 || !positive_finite(focal)) return SN_E_BADARG;
  return sn_ndc_rays_launch(rays_in, n_rays, ndc_scale(W, focal), ndc_scale(H, focal), ndc_near, rays_out, nullptr, H, W,
                            (hipStream_t)stream);
}

int sn_ndc_rays_backward(const float* rays_in, const float* g_rays_out, long n_rays, int H, int W, float focal, float ndc_near,
                         float* g_rays_in, void* stream) {
  if (!rays_in || !g_rays_out || !g_rays_in || n_rays < 0 || H < 1 || W < 1 || !positive_finite(focal)) return SN_E_BADARG;
  return sn_ndc_rays_backward_launch(rays_in, g_rays_out, n_rays, ndc_scale(W, focal), ndc_scale(H, focal), ndc_near, g_rays_in,
                                     nullptr, H, W, nullptr, nullptr, (hipStream_t)stream);
}

// ---- the same with the intrinsics in DEVICE memory: their values are not looked at on the host (that would be a sync); everything
// else is checked as above (check_camera with focal lengths that pass)
int sn_generate_rays_cam_dev(const float* c2w, const float* intr, int H, int W, int convention, int ndc, float ndc_near, float near,
                             float far, int x0, int y0, int stride_x, int stride_y, int patch_w, int patch_h, float* rays,
                             void* stream) {
  if (!c2w || !intr || !rays) return SN_E_BADARG;
  if (const int refused = check_camera(H, W, 1.0f, 1.0f, convention, ndc, 1.0f, x0, y0, stride_x, stride_y, patch_w, patch_h))
    return refused;
  return sn_generate_rays_cam_launch(c2w, 1.0f, 1.0f, 0.0f, 0.0f, convention, ndc, 0.0f, 0.0f, ndc_near, near, far, x0, y0, stride_x,
                                     stride_y, patch_w, patch_h, rays, intr, H, W, (hipStream_t)stream);
}

long sn_camera_backward_workspace_bytes(void) { return sn_camera_backward_workspace_bytes_impl(); }

int sn_generate_rays_cam_dev_backward(const float* g_rays, const float* c2w, const float* intr, int H, int W, int convention, int ndc,
                                      float ndc_near, int x0, int y0, int stride_x, int stride_y, int patch_w, int patch_h,
                                      void* workspace, float* g_c2w, float* g_intr, void* stream) {
  if (!g_rays || !c2w || !intr || !workspace || (!g_c2w && !g_intr)) return SN_E_BADARG;
  if (const int refused = check_camera(H, W, 1.0f, 1.0f, convention, ndc, 1.0f, x0, y0, stride_x, stride_y, patch_w, patch_h))
    return refused;
  return sn_generate_rays_cam_backward_launch(g_rays, c2w, 1.0f, 1.0f, 0.0f, 0.0f, convention, ndc, 0.0f, 0.0f, ndc_near, x0, y0,
                                              stride_x, stride_y, patch_w, patch_h, workspace, g_c2w, intr, H, W, g_intr,
                                              (hipStream_t)stream);
}

int sn_ndc_rays_dev(const float* rays_in, long n_rays, int H, int W, const float* focal, float ndc_near, float* rays_out,
                    void* stream) {
  if (!rays_in || !rays_out || !focal || n_rays < 0 || H < 1 || W < 1) return SN_E_BADARG;
  return sn_ndc_rays_launch(rays_in, n_rays, 0.0f, 0.0f, ndc_near, rays_out, focal, H, W, (hipStream_t)stream);
}

int sn_ndc_rays_dev_backward(const float* rays_in, const float* g_rays_out, long n_rays, int H, int W, const float* focal,
                             float ndc_near, void* workspace, float* g_rays_in, float* g_focal, void* stream) {
  if (!rays_in || !g_rays_out || !focal || !workspace || !g_rays_in || !g_focal || n_rays < 0 || H < 1 || W < 1) return SN_E_BADARG;
  return sn_ndc_rays_backward_launch(rays_in, g_rays_out, n_rays, 0.0f, 0.0f, ndc_near, g_rays_in, focal, H, W, workspace, g_focal,
                                     (hipStream_t)stream);
}

int sn_composite_forward(const float* raw, int has_rgb, const float* z_vals, const float* rays, const float* noise,
                         float noise_std, long n_rays, int n_samples, int white_back, float* rgb, float* depth,
                         float* weights, void* stream) {
  if (!raw || !z_vals || !rays || !weights || n_rays < 0 || n_samples < 1) return SN_E_BADARG;
  if (has_rgb && (!rgb || !depth)) return SN_E_BADARG;
  return sn_composite_forward_launch(raw, has_rgb, z_vals, rays, noise, noise_std, n_rays, n_samples, white_back, rgb,
                                     depth, weights, (hipStream_t)stream);
}

int sn_sample_pdf(const float* z_vals, const float* weights, const float* u, long n_rays, int n_samples,
                  int n_importance, float* z_fine, float* z_merged, void* stream) {
  if (!z_vals || !weights || !z_merged || n_rays < 0) return SN_E_BADARG;
  return sn_sample_pdf_launch(z_vals, weights, u, n_rays, n_samples, n_importance, z_fine, z_merged, (hipStream_t)stream);
}

int sn_sample_pdf_bins(const float* bins, const float* weights, const float* u, long n_rays, int n_bins,
                       int n_importance, float eps, float* samples, void* stream) {
  if (!bins || !weights || !samples || n_rays < 0 || !(eps > 0.0f)) return SN_E_BADARG;
  return sn_sample_pdf_bins_launch(bins, weights, u, n_rays, n_bins, n_importance, eps, samples, (hipStream_t)stream);
}

}  // extern "C"
