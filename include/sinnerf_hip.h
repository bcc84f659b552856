/* sinnerf_hip.h -- C ABI of libsinnerf_hip.so: the MI355X (gfx950) volume-rendering hot path of SinNeRF.
 *
 * The reference (VITA-Group/SinNeRF) has no FFI: its hot path is Python calling ATen ops
 * (models/rendering.py::render_rays, models/nerf.py::{Embedding,NeRF}).  Each entry point below replaces the
 * group of reference lines cited next to it; sinnerf_amd/rendering.py (the drop-in render_rays) binds them
 * with ctypes -- see INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions: every pointer is a DEVICE pointer unless the name ends in _host; tensors are dense row-major
 * fp32; `stream` is a hipStream_t passed as void* (NULL = default stream).  Functions only enqueue work: no
 * allocation, no synchronisation, no global state (one exception: the fp32 inference launches of sn_mlp_forward /
 * sn_mlp_forward_embedded draw their work units from a library-owned device word per stream, zeroed on the stream
 * in front of every launch -- a memset node when captured; at most 2^31 - 1 units of 32 points, SN_E_TOOLARGE
 * beyond).  Return 0 on success, a negative SN_E_* code for argument
 * errors, a positive value = hipError_t of a failed launch.
 */
#ifndef SINNERF_HIP_H
#define SINNERF_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SN_ABI_VERSION 5   /* 2: sn_sample_pdf_bins gained eps, dtype carries SN_DTYPE_CLASSIC_HEADS, sn_mlp_forward flag bits
                            * 3: dtype carries SN_DTYPE_COMPILER_SCHEDULED and SN_DTYPE_EMB_BF16
                            * 4: SN_DTYPE_BF16X3 (inference and training entries, packers), sn_pack_table_entries_dtype
                            * 5: SN_DTYPE_F16 (inference entries, packer), SN_FLAG_F32_LDS_RING
                            *    (additive within 5: the pose-gradient entries sn_ray_grads, sn_ray_grads_workspace_bytes,
                            *    sn_composite_backward_rays, sn_generate_rays_backward and its workspace query; the camera entries
                            *    sn_generate_rays_cam, sn_generate_rays_cam_backward, sn_ndc_rays, sn_ndc_rays_backward
                            *    and, with the intrinsics in device memory and their gradients, sn_generate_rays_cam_dev,
                            *    sn_generate_rays_cam_dev_backward, sn_camera_backward_workspace_bytes, sn_ndc_rays_dev,
                            *    sn_ndc_rays_dev_backward; the density-gradient entries sn_point_grads, sn_point_grads_wsum) */

#define SN_DTYPE_F32 0  /* v_mfma_f32_32x32x2_f32, exact fp32                                          */
#define SN_DTYPE_BF16 1 /* v_mfma_f32_32x32x16_bf16, bf16 operands / fp32 accumulate                    */
#define SN_DTYPE_BF16_STATE 2 /* training entries only: SN_DTYPE_BF16 arithmetic AND acts / g_acts stored as bf16
                               * (same shapes; the float* parameters then point at bf16 arrays; emb stays fp32
                               * unless SN_DTYPE_EMB_BF16 is OR-ed in)                                             */
#define SN_DTYPE_BF16X3 3 /* sn_mlp_forward, sn_mlp_forward_embedded, sn_mlp_forward_train[_embedded], sn_mlp_backward_chain,
                           * sn_weight_grads (training state: see sn_mlp_forward_train) and the packer: fp32-LEVEL accuracy on the bf16
                           * MFMA -- every weight and activation as a (hi, lo) bf16 pair, W.x ~= Wh.xh + Wl.xh + Wh.xl with fp32
                           * accumulation (3 bf16 MFMAs instead of 8 fp32 ones per 16 k; SURVEY §7 "3-term bf16 split"); exact
                           * embeddings and fp32 heads as SN_DTYPE_F32.  Measured against the fp32 bars of the parity tests.  */
/* OR-ed into `dtype` of the sn_mlp_* entry points: the network was built as NeRF(use_new_activation=False), the
 * constructor's default (models/nerf.py:47-50, :91-100) -- ReLU after dir_encoding, Sigmoid after rgb -- instead of the
 * ShiftedSoftplus / WidenedSigmoid heads both reference call sites ask for (models/nerf.py:81-90, models/activations.py).
 * Blobs, training state and every other entry point are the same for both.                                          */
#define SN_DTYPE_F16 4 /* ABI 5. sn_mlp_forward, sn_mlp_forward_embedded, sn_pack_weights only (INFERENCE): v_mfma_f32_32x32x16_f16,
                        * fp16 operands (11 significand bits instead of bf16's 8) / fp32 accumulate at the bf16 matrix rate -- the
                        * instruction streams of SN_DTYPE_BF16 with v_cvt_pk_f16_f32.  On the trained-weight fixtures its error is
                        * 8-17x below SN_DTYPE_BF16's (tests/test_trained_weights_gpu.py); activations beyond +-65504 overflow (the
                        * entry points do not check).  Blob layout and size = SN_DTYPE_BF16's. */
#define SN_DTYPE_CLASSIC_HEADS 0x100
/* OR-ed into `dtype` of sn_mlp_forward_train / sn_mlp_backward_chain: run the PREVIOUS generation of the kernel instead of the shipped one --
 * SN_DTYPE_BF16_STATE / SN_DTYPE_BF16X3: the compiler-scheduled kernels (csrc/sn_mlp_fwd_bf16.hip, csrc/sn_mlp_bwd_bf16.hip,
 * csrc/sn_mlp_{fwd,bwd}_bf16x3.hip) instead of the generated instruction streams (csrc/sn_mlp_*_t.hip); SN_DTYPE_F32 (round 6): the
 * LDS-ring kernels (csrc/sn_mlp_fwd.hip, csrc/sn_mlp_bwd.hip) instead of the fragments-from-L2 ones (csrc/sn_mlp_fwd_f32g.hip,
 * csrc/sn_mlp_bwd_f32g.hip).  Same arithmetic, same stored state bit for bit; kept for A/B timing and the bit-identity tests. */
#define SN_DTYPE_COMPILER_SCHEDULED 0x200
/* OR-ed into `dtype` (SN_DTYPE_BF16_STATE, hand-scheduled kernels) of sn_mlp_forward_train, sn_weight_grads and
 * sn_weight_grads_workspace_bytes -- all three or none: `emb` is a bf16 array (slot_rows, 128) holding the embedded inputs as the
 * MFMA operands the forward builds, in its K-slot order instead of the reference's column order: positions [0, 64) =
 * Embedding(xyz) (lane half h, slot e at 32 h + e), [64, 96) = Embedding(dir) (16 h + e), [96, 128) never written.  192 B per point
 * instead of 360 B written, half the bytes read by the three contractions that use it; sn_weight_grads returns the same gradients bit
 * for bit (it contracts the same bf16 values in the same order and permutes the 63 / 27 columns back).              */
#define SN_DTYPE_EMB_BF16 0x400

#define SN_E_BADARG (-1)
#define SN_E_TOOLARGE (-2)
#define SN_E_MISSING_RNG (-3)
#define SN_E_UNSUPPORTED (-4)
#define SN_E_BADSHAPE (-5)

/* sn_mlp_forward `flags` (sn_mlp_forward_embedded: reserved, pass 0):
 * bit 1: dtype SN_DTYPE_BF16 only -- run the compiler-scheduled kernel (csrc/sn_mlp_fwd_bf16.hip) instead of the
 * hand-scheduled one (csrc/sn_mlp_fwd_bf16_v3.hip); same arithmetic, kept for A/B timing and as the sigma-only / training form. */
#define SN_FLAG_BF16_COMPILER_SCHEDULED 2
/* bit 2: dtype SN_DTYPE_F32 only -- run the round-1..5 inference kernel (csrc/sn_mlp_fwd.hip: weights through an LDS ring filled by
 * LDS-DMA, one barrier per slab) instead of the round-6 one (csrc/sn_mlp_fwd_f32g.hip: A fragments straight from L2 into a register
 * ring, no VALU instruction in the trunk, no barrier); bit-identical results for non-NaN activations (the round-6 kernels take the
 * ReLU as ds_max_i32 against 0, which turns a negative NaN into 0 and keeps a positive one, where v_max_f32 gives 0 for both -- the
 * same caveat holds for SN_DTYPE_F32 | SN_DTYPE_COMPILER_SCHEDULED above); kept for A/B timing.  Also honoured by
 * sn_mlp_forward_embedded. */
#define SN_FLAG_F32_LDS_RING 4

int sn_abi_version(void);
const char* sn_error_string(int code);

/* kernel routing introspection (host only like the sn_layout_* entries: no device call, no allocation; additive within ABI 5; used by
 * tests/test_api_routing_cpu.py).  The launcher the MLP entry `entry` hands (dtype, flags, sigma_only, n_points) to, as its symbol
 * name without "_launch" (e.g. "sn_mlp_forward_bf16_v3_classic"), or NULL where that entry refuses the dtype with SN_E_UNSUPPORTED.
 * `flags` and `sigma_only` count for the two inference entries only, `n_points` for the training ones. */
#define SN_ROUTE_FORWARD 0          /* sn_mlp_forward */
#define SN_ROUTE_FORWARD_EMBEDDED 1 /* sn_mlp_forward_embedded */
#define SN_ROUTE_TRAIN 2            /* sn_mlp_forward_train */
#define SN_ROUTE_TRAIN_EMBEDDED 3   /* sn_mlp_forward_train_embedded */
#define SN_ROUTE_CHAIN 4            /* sn_mlp_backward_chain */
const char* sn_mlp_route(int entry, int dtype, int flags, int sigma_only, long n_points);

/* layout introspection (host only; mirrors csrc/sn_layout.h -- used by the CPU layout tests) */
int sn_layout_xyz_slot_col(int lane_half, int slot); /* reference Embedding(3,10) column, -1 = zero pad */
int sn_layout_dir_slot_col(int lane_half, int slot); /* reference Embedding(3,4) column, -1 = zero pad  */
int sn_layout_slab_k(int slab);
int sn_layout_n_slabs(void);

/* ---- weights -------------------------------------------------------------------------------------------
 * One NeRF MLP (models/nerf.py:66-103, NeRF(D=8,W=256,63,27,skips=[4],use_new_activation=True)) is consumed by
 * the kernels as a "packed blob": weights reordered into MFMA A-fragment order (csrc/sn_layout.h).
 * raw[24] = device pointers of the state_dict tensors in this order (names = nerf.py:75-103):
 *   xyz_encoding_{1..8}.0.weight/.bias (16), xyz_encoding_final.weight/.bias, dir_encoding.0.weight/.bias,
 *   sigma.weight/.bias, rgb.0.weight/.bias                                                              */
#define SN_N_RAW_TENSORS 24
long sn_packed_weights_bytes(int dtype);
long sn_pack_table_entries(void);           /* SN_DTYPE_F32 / SN_DTYPE_BF16 */
long sn_pack_table_entries_dtype(int dtype); /* any packable dtype (SN_DTYPE_BF16X3 has two entries per weight) */
/* fills table_host[2*entries] int32 (dst byte offset, src tensor<<20|offset or -1); upload it once */
int sn_build_pack_table(int dtype, int32_t* table_host);
int sn_pack_weights(const float* const* raw_host_array_of_device_ptrs, const int32_t* table, long n_entries,
                    void* blob, int dtype, void* stream);
/* transposed-weight blob consumed by sn_mlp_backward_chain (fp32; same table format, same packer) */
long sn_packed_weights_bytes_bwd(void);
long sn_pack_table_entries_bwd(void);
int sn_build_pack_table_bwd(int32_t* table_host);
/* ... and its bf16-operand form (sn_mlp_backward_chain with dtype SN_DTYPE_BF16; pack with sn_pack_weights(..., SN_DTYPE_BF16)) */
long sn_packed_weights_bytes_bwd_bf16(void);
long sn_pack_table_entries_bwd_bf16(void);
int sn_build_pack_table_bwd_bf16(int32_t* table_host);
/* ... and its bf16x3 form (sn_mlp_backward_chain with dtype SN_DTYPE_BF16X3; pack with sn_pack_weights(..., SN_DTYPE_BF16X3)) */
long sn_packed_weights_bytes_bwd_bf16x3(void);
long sn_pack_table_entries_bwd_bf16x3(void);
int sn_build_pack_table_bwd_bf16x3(int32_t* table_host);

/* ---- models/rendering.py:264-282  z_vals = near*(1-t)+far*t (or disparity), stratified perturb -----------
 * rays (n_rays,8) = [o(3), d(3), near, far] (rendering.py:257-258); perturb_rand (n_rays,n_samples) = the
 * torch.rand draw of :281 (required iff perturb > 0); z_vals out (n_rays,n_samples).                      */
int sn_sample_coarse(const float* rays, long n_rays, int n_samples, int use_disp, float perturb,
                     const float* perturb_rand, float* z_vals, void* stream);

/* ---- models/rendering.py:187-212 (closure `inference`, MLP part) + models/nerf.py:36-41,122-148 -----------
 * For every sample point p = (ray, i): xyz = o + d*z (rendering.py:284-285), Embedding(xyz) (63), Embedding(d)
 * (27), NeRF.forward.  out: (n_rays*n_samples, 4) = [rgb, raw sigma] (nerf.py:146), or (n_rays*n_samples)
 * raw sigma when sigma_only (nerf.py:136-138).  Replaces the chunk loop of rendering.py:196-206.           */
int sn_mlp_forward(const void* blob, int dtype, const float* rays, const float* z_vals, long n_rays, int n_samples,
                   int sigma_only, int flags, float* out, void* stream);

/* ---- training forward: sn_mlp_forward + the activations autograd would keep alive --------------
 * dtype SN_DTYPE_BF16 = mixed precision: bf16-operand contractions as in sn_mlp_forward, fp32 activations stored (the
 * values before their bf16 rounding) for the fp32 backward.
 * slot_rows = rows allocated per slot, >= n_points rounded up to a multiple of 128 (fp32) / 256 (bf16): the kernel stores
 * whole point tiles without a predicate (rows >= n_points receive finite copies of the last point; their gradients are zero, so
 * sn_dw_gemm, which walks whole 16-point chunks, ignores them).
 * acts (10, slot_rows, 256): slots 0..7 = outputs of xyz_encoding_1..8 (post-ReLU), 8 = xyz_encoding_final,
 * 9 = dir_encoding output (128 wide, leading dimension 256).  emb (slot_rows, 128): the kernel writes columns
 * [0,63) = Embedding(xyz) and [64,91) = Embedding(dir) in the reference's column order (nerf.py:36-41) of every row
 * of the whole point tiles; columns 63 and 91..127 are never written (nor read back by sn_weight_grads' results:
 * zero-fill them only if you contract emb yourself).
 * SN_DTYPE_BF16_STATE: the unused half of slot 9 (columns 128..255 of the bf16 array, 256 B per point) receives the ReLU
 * SIGN WORDS of xyz_encoding_1..8 -- for the 64 consecutive points a wave owns, the 32-bit word of (layer l, 32-feature
 * tile t) and lane L sits in row (first point + 8 l + t), bytes [256 + 4 L, 256 + 4 L + 4).  sn_mlp_backward_chain with
 * SN_DTYPE_BF16_STATE takes its ReLU masks from these words (and reads no other activation but slot 9's values): pass it
 * the acts array THIS entry wrote.
 * SN_DTYPE_BF16X3: buffers of the fp32 shapes and sizes (slot_rows a multiple of 128).  emb and slot 9 are fp32 exactly as above;
 * SLOTS 0..8 hold every value as the (hi, lo) bf16 PAIR the kernels compute with -- hi = RNE(x), lo = RNE(x - hi), x = hi + lo to
 * 2^-17 relative -- in the 1 KB an fp32 row takes: per 8 consecutive features 16 B of hi parts, then 16 B of lo parts (feature f of a
 * row: hi at byte 32 (f / 8) + 2 (f % 8), lo 16 B further).  sn_mlp_backward_chain writes slots 0..8 of g_acts the same way,
 * sn_weight_grads reads both (no conversion on its way to the MFMA).  The unused half of slot 9 receives ReLU sign words for the
 * chain as with SN_DTYPE_BF16_STATE, in this kernel's tile shape: for the 32 points a wave owns, layer l sits in rows
 * first point + 4 l + (lane >> 4), bytes [512 + 16 (lane & 15), + 16) -- one word per lane and pair of 32-feature tiles.      */
int sn_mlp_forward_train(const void* blob, int dtype, const float* rays, const float* z_vals, long n_rays, int n_samples,
                         float* out, float* acts, float* emb, long slot_rows, void* stream);

/* ---- the same for NeRF.forward(x) under autograd (models/nerf.py:105-148 is an ordinary differentiable nn.Module): x
 * (n_rows, ld >= 90) pre-embedded rows as for sn_mlp_forward_embedded; acts / slot_rows as above.  The `emb` matrix of the
 * weight-gradient contractions is a column re-layout of x the caller builds itself ([0,63) = x[:, 0:63], [64,91) =
 * x[:, 63:90], zeros elsewhere).  dtype: SN_DTYPE_F32 or SN_DTYPE_BF16_STATE.                                   */
int sn_mlp_forward_train_embedded(const void* blob, int dtype, const float* x, long n_rows, int ld, float* out,
                                  float* acts, long slot_rows, void* stream);

/* ---- backward of models/nerf.py:122-148 w.r.t. layer outputs (what loss.backward() at sinnerf.py:551 runs) ----
 * blob_bwd: transposed-weight blob (sn_build_pack_table_bwd).  out_raw / g_raw (n_points,4): forward output and its
 * gradient.  Writes g_acts (10, slot_rows, 256): slots 0..7 = dL/d(pre-activation) of xyz_encoding_1..8, 8 = of
 * xyz_encoding_final, 9 = of dir_encoding (128 wide); g_out (n_points,4) = dL/d(pre-activation) of rgb (3), sigma (1).
 * dtype SN_DTYPE_BF16: blob_bwd from the *_bwd_bf16 table, bf16-operand contractions, everything stored stays fp32.
 * dtype SN_DTYPE_BF16X3: blob_bwd from the *_bwd_bf16x3 table; fp32-level accuracy on the bf16 MFMA (3-term hi/lo split); acts as
 * sn_mlp_forward_train(SN_DTYPE_BF16X3) wrote them (masks from the sign words, h2 from slot 9), g_acts in the same layout: slots 0..8
 * as (hi, lo) pairs, slot 9 (128 columns + the head block) fp32 (slot_rows a multiple of 128).
 * dtype SN_DTYPE_BF16_STATE: acts / g_acts are bf16 arrays; the ReLU masks come from the sign words sn_mlp_forward_train
 * left in slot 9 (see there), gradients leave as whole 128-byte rows.
 * slot_rows as for sn_mlp_forward_train (>= n_points rounded up to 128, 256 for bf16; rows >= n_points of slots' 256
 * columns are written as zeros, the caller zero-fills the rest of the pad rows).  Weight gradients are the contractions  dW_l = g_l^T X_l  over points of these matrices with acts / emb.
 * PAIRING RULE (all three training entry points): the state arrays of the arithmetics have the same shapes and byte sizes but NOT the
 * same contents -- `acts` written by sn_mlp_forward_train(dtype D) may only be read by sn_mlp_backward_chain(D) and sn_weight_grads(D),
 * `g_acts` written by sn_mlp_backward_chain(D) only by sn_weight_grads(D), with D one of {SN_DTYPE_F32 (also read by SN_DTYPE_BF16),
 * SN_DTYPE_BF16_STATE, SN_DTYPE_BF16X3}.  The library cannot tell the layouts apart from the pointers: a mismatch (e.g. an x3 state
 * handed to the SN_DTYPE_F32 chain) yields wrong gradients, not an error code.  SN_DTYPE_BF16X3 additionally requires slot_rows % 128 == 0
 * (checked: SN_E_BADSHAPE).                                                                                                            */
int sn_mlp_backward_chain(const void* blob_bwd, int dtype, const float* acts, const float* out_raw, const float* g_raw,
                          long n_points, long slot_rows, float* g_acts, float* g_out, void* stream);

/* ---- weight gradients  dW[m,n] = sum_p G[p,m] X[p,n],  db[m] = sum_p G[p,m]  (autograd of every nn.Linear of
 * models/nerf.py:66-103: gW = g_y^T x, gb = sum g_y) as K-split MFMA contractions over all sample points.
 * tasks: DEVICE array of n_tasks 64-byte records (one workgroup each):
 *   { const float* a;  const float* b;  float* c;  float* bias_or_NULL;  int64 k0, k1;  int32 lda, ldb;  int32 ldc, variant; }
 * a = G + column offset (row-major [P][lda]), b = X + column offset ([P][ldb]), point range [k0,k1) with
 * (k1-k0) % 16 == 0 and every row readable (zero-padded G rows contribute nothing);
 * variant 0: M x N = 256x256, 1: 256x64, 2: 128x256, 3: 128x64.  c receives the PARTIAL M x N result of that K-range
 * (row-major, leading dimension ldc), bias the partial column sums of a; the caller sums the partials of a problem. */
int sn_dw_gemm(const void* tasks, int n_tasks, void* stream);

/* ---- ALL weight / bias gradients of one NeRF from the stored training state, as two launches with nothing built on the
 * host (capturable in a HIP graph): the 14 contractions above (K-split over ~one workgroup per CU by a per-mode cost model,
 * described to the kernel BY VALUE in its arguments), then one kernel that sums the K-split partials in a fixed order
 * (deterministic, no atomics) and writes the results in the parameters' own shapes -- what autograd hands to
 * nn.Linear.weight.grad / .bias.grad for models/nerf.py:66-103 (the cat of the skip / direction inputs, nerf.py:133,142,
 * becomes two column ranges of the same gradient).
 *   acts, emb: as written by sn_mlp_forward_train; g_acts: as written by sn_mlp_backward_chain (pad rows zero);
 *   slot_rows: any multiple of 16, >= 16; dtype: SN_DTYPE_F32 (fp32 MFMAs), SN_DTYPE_BF16 (bf16 operands, fp32 state) or
 *   SN_DTYPE_BF16_STATE (acts / g_acts stored as bf16) or SN_DTYPE_BF16X3 (the x3 state; see the PAIRING RULE at sn_mlp_backward_chain:
 *   acts / g_acts must have been written with the SAME dtype);
 *   workspace: sn_weight_grads_workspace_bytes(slot_rows, dtype) bytes of DEVICE scratch (the K-split partials);
 *   grads: HOST array of SN_N_RAW_TENSORS device pointers in the order of sn_pack_weights' `raw` (NULL = not wanted);
 *   accumulate != 0: grads[i] += result (autograd's accumulation into an existing .grad), else grads[i] = result.
 * Pinned by tests/test_dw_plan_cpu.py and tests/test_weight_grads_edges_gpu.py:
 *   - ANY slot_rows that is a multiple of 16 and at least 16 is supported (not only the multiples of 128 / 256 the training forward
 *     asks for): every point is contracted exactly once, whatever the K-split makes of the size;
 *   - the workspace need NOT be initialised: every task writes its whole partial before the finish kernel sums it (no K-range of the
 *     plan is empty), so stale contents -- NaN bit patterns included -- never reach a gradient;
 *   - the columns of `emb` the training forward never writes (fp32 form: 63 and 91..127; SN_DTYPE_EMB_BF16: the positions no column
 *     maps to and [96, 128)) may hold anything, NaN included: they are staged with their rows but no gradient depends on them.          */
long sn_weight_grads_workspace_bytes(long slot_rows, int dtype);
/* The plan sn_weight_grads runs for (slot_rows, dtype), for tests and tools (host only like the sn_layout_* entries: no device call, no
 * allocation; argument checks and error codes of sn_weight_grads_workspace_bytes, SN_E_BADARG for max_probs < 0 or a null out_host with
 * max_probs > 0).  Returns the number of problems (14) and writes, for the first max_probs of them in launch order, 9 int32:
 *   { variant | flag bits (the `variant` of sn_dw_gemm's task record), m, n, ns, per, launch group, first task in group,
 *     c_off / 256, b_off / 256 or -1 }
 * -- problem q is the m x n contraction split into ns K-ranges [j per, min((j + 1) per, slot_rows)), run by tasks first + j of launch
 * `group`, partial j at workspace byte c_off + j m n 4 (column sums: b_off + j m 4; -1 = none).  Coverage property: per % 16 == 0 and
 * (ns - 1) per < slot_rows <= ns per, i.e. every point lies in exactly one range and no range is empty.                              */
int sn_weight_grads_plan(long slot_rows, int dtype, int32_t* out_host, int max_probs);
int sn_weight_grads(const void* acts, const float* emb, const void* g_acts, long slot_rows, int dtype, void* workspace,
                    float* const* grads_host_array_of_device_ptrs, int accumulate, void* stream);

/* ---- backward of models/rendering.py:215-246 w.r.t. raw=[rgb,sigma]; g_rgb (n_rays,3), g_depth (n_rays),
 * g_weights (n_rays,n_samples) are upstream gradients (any may be NULL = zeros); g_raw (n_rays,n_samples,4).  */
int sn_composite_backward(const float* raw, const float* z_vals, const float* rays, const float* noise, float noise_std,
                          long n_rays, int n_samples, int white_back, const float* g_rgb, const float* g_depth,
                          const float* g_weights, float* g_raw, void* stream);

/* ==== gradients with respect to the RAYS (additive within ABI 5) ==============================================
 * The reference's render_rays is an ordinary differentiable function of its rays (pose refinement, iNeRF-style registration);
 * the three entries below are what autograd derives for one render pass with z_vals held constant (the coarse depths depend on
 * near / far only, rendering.py:264-282; the fine ones are detached at :312).  near / far themselves (columns 6, 7) are treated as
 * constants: their gradient columns are written as zeros.
 *
 * ---- backward of models/nerf.py:36-41 (Embedding) + :122-148 (the three layers that read the embedded input) + the point
 * construction xyz = o + d z, dir = d of rendering.py:187-190, :284-285, summed over the samples of each ray:
 *   g_emb_xyz = G0 . W1 + G4 . W5[:, 0:63]   (nerf.py:133: the skip input is cat([input_xyz, h]))
 *   g_emb_dir = G9[:, 0:128] . Wdir[:, 256:283]   (nerf.py:142: cat([xyz_encoding_final, input_dir]))
 *   g_x = ge[0:3] + sum_k 2^k (cos(2^k x) ge[3+6k : 6+6k] - sin(2^k x) ge[6+6k : 9+6k])   (k < 10 at xyz, k < 4 at d; sin / cos recomputed)
 *   g_rays[r, 0:3] = sum_s g_xyz[r, s]       g_rays[r, 3:6] = sum_s z[r, s] g_xyz[r, s] + sum_s g_dirvec[r, s]       g_rays[r, 6:8] = 0
 * w1 = xyz_encoding_1.0.weight (256 x 63), w5 = xyz_encoding_5.0.weight (256 x 319), wdir = dir_encoding.0.weight (128 x 283): the raw
 * fp32 parameter tensors, row-major (no packed blob).  g_acts / slot_rows: as written by sn_mlp_backward_chain; only slots 0, 4 and 9
 * and only rows < n_rays * n_samples are read.  dtype names the LAYOUT that chain left: SN_DTYPE_F32 / SN_DTYPE_BF16 (fp32 rows),
 * SN_DTYPE_BF16_STATE (bf16 rows), SN_DTYPE_BF16X3 (slots 0 and 4 as (hi, lo) pairs -- the value used is hi + lo -- slot 9 fp32); anything
 * else, flag bits included, is SN_E_UNSUPPORTED.  The arithmetic is fp32 (v_mfma_f32_32x32x2_f32) whatever the layout.
 * g_rays (n_rays, 8) is WRITTEN (not accumulated); the sums over samples run in a fixed order without atomics, so two calls give the
 * same bits.  n_samples in 1..1024.  workspace: sn_ray_grads_workspace_bytes(n_rays, n_samples) bytes of DEVICE scratch.
 * The compositor's own contribution to g_rays[:, 3:6] (through ||d||) comes from sn_composite_backward_rays; add the two.     */
long sn_ray_grads_workspace_bytes(long n_rays, int n_samples);
int sn_ray_grads(const float* w1, const float* w5, const float* wdir, int dtype, const void* g_acts, long slot_rows,
                 const float* rays, const float* z_vals, long n_rays, int n_samples, void* workspace, float* g_rays,
                 void* stream);

/* ---- sn_composite_backward + the gradient through deltas = dz * ||d|| (models/rendering.py:215-222, :228):
 *   dL/d||d|| = sum_i dL/dalpha_i exp(-delta_i s_i) max(sigma_i + noise_i, 0) dz_i     (dz_i = z_{i+1} - z_i, 1e10 for the last sample)
 *   g_rays[r, 3:6] = dL/d||d|| * d / ||d||   (0 for a ray with ||d|| = 0),   every other column 0.
 * g_raw receives the same bits sn_composite_backward writes (one kernel body); g_rays (n_rays, 8) is written.                   */
int sn_composite_backward_rays(const float* raw, const float* z_vals, const float* rays, const float* noise, float noise_std,
                               long n_rays, int n_samples, int white_back, const float* g_rgb, const float* g_depth,
                               const float* g_weights, float* g_raw, float* g_rays, void* stream);

/* ==== gradients with respect to a POSITION (additive within ABI 5) ============================================
 * What autograd derives from models/nerf.py:36-41 + :122-148 for d(out)/d(xyz) at every sample point, kept PER POINT: the
 * contraction and the Embedding derivative of sn_ray_grads without its direction part and without its sum over the samples of a ray.
 *   g_emb_xyz = G0 . W1 + G4 . W5[:, 0:63]
 *   g_xyz[p]  = ge[0:3] + sum_k 2^k (cos(2^k x) ge[3+6k : 6+6k] - sin(2^k x) ge[6+6k : 9+6k])   (k < 10; sin / cos recomputed)
 * (sin / cos from the forward's range reduction with its one rounding compensated, so a factor near one of its zeros keeps its
 * relative accuracy: a per-point gradient has no sum over samples behind which an absolute 2e-7 of the angle could hide)
 * at x = fl(o + fl(d z)), the fp32 position the forward embedded (rendering.py:284-285), p = (ray, sample) in row order.  With g_acts
 * from sn_mlp_backward_chain run on g_raw = (0, 0, 0, 1) for every point this is the gradient of the raw sigma (nerf.py:136), the
 * un-normalised surface normal up to sign; any other g_raw gives the position gradient of that linear functional of the output.
 * w1, w5: the raw fp32 parameter tensors as for sn_ray_grads.  g_acts / slot_rows: as written by sn_mlp_backward_chain; only slots 0
 * and 4 and only rows < n_rays * n_samples are read (pad rows may hold anything, NaN included).  dtype names the LAYOUT that chain left,
 * exactly as for sn_ray_grads: SN_DTYPE_F32 / SN_DTYPE_BF16 (fp32 rows), SN_DTYPE_BF16_STATE (bf16 rows), SN_DTYPE_BF16X3 ((hi, lo)
 * pairs, the value used is hi + lo); anything else, flag bits included, is SN_E_UNSUPPORTED.  fp32 arithmetic
 * (v_mfma_f32_32x32x2_f32) whatever the layout.  g_xyz (n_rays * n_samples, 4) = [gx, gy, gz, 0] is WRITTEN (not accumulated), one
 * 16-byte store per point; no atomics, no workspace: two calls give the same bits.  n_samples in 1..1024 (SN_E_BADSHAPE), slot_rows >=
 * n_rays * n_samples (SN_E_BADSHAPE), a null pointer is SN_E_BADARG; n_rays <= 0 launches nothing and returns 0.                    */
int sn_point_grads(const float* w1, const float* w5, int dtype, const void* g_acts, long slot_rows, const float* rays,
                   const float* z_vals, long n_rays, int n_samples, float* g_xyz, void* stream);

/* ---- the weighted sum of the per-point gradients over the samples of each ray (the numerator of a normal map):
 *   g_sum[r] = [sum_s weights[r, s] g_xyz[r, s, 0:3], 0]
 * g_xyz (n_rays * n_samples, 4) as written by sn_point_grads, weights (n_rays, n_samples) e.g. the compositing weights of
 * sn_composite_forward.  One wave per ray: products and sums in fp64 (a product of two fp32 values is exact there), lane l adds samples
 * l, l + 64, ... in order, then a butterfly over the lanes; ONE rounding to fp32.  Fixed order, no atomics: two calls give the same
 * bits.  g_sum (n_rays, 4) is written.  n_samples in 1..1024 (SN_E_BADSHAPE); a null pointer is SN_E_BADARG; n_rays <= 0 launches
 * nothing and returns 0.                                                                                                     */
int sn_point_grads_wsum(const float* g_xyz, const float* weights, long n_rays, int n_samples, float* g_sum, void* stream);

/* ---- models/nerf.py:105-148  NeRF.forward(x, sigma_only) on an already embedded matrix --------------------
 * x (n_rows, ld) with columns [0,63) = embedded xyz and [63,90) = embedded dir (ignored when sigma_only).   */
int sn_mlp_forward_embedded(const void* blob, int dtype, const float* x, long n_rows, int ld, int sigma_only,
                            int flags, float* out, void* stream);

/* ---- models/rendering.py:215-246  deltas, noise, alpha, cumprod transmittance, weights, rgb/depth/white_back
 * raw: (n_rays,n_samples,4) if has_rgb else (n_rays,n_samples) raw sigma (weights_only, rendering.py:238-239)
 * noise: (n_rays,n_samples) torch.randn draw of :224 or NULL (= zeros).  rgb (n_rays,3), depth (n_rays) are
 * written only when has_rgb; weights (n_rays,n_samples) always.                                           */
int sn_composite_forward(const float* raw, int has_rgb, const float* z_vals, const float* rays, const float* noise,
                         float noise_std, long n_rays, int n_samples, int white_back, float* rgb, float* depth,
                         float* weights, void* stream);

/* ---- models/rendering.py:15-61 (sample_pdf) + :310-315 (mid points, detach, cat + sort) -------------------
 * z_vals/weights (n_rays,n_samples) coarse depths / compositing weights; u (n_rays,n_importance) = torch.rand
 * draw of :43 or NULL for det=True (linspace, :40).  z_fine (n_rays,n_importance) optional (may be NULL),
 * z_merged (n_rays, n_samples+n_importance) ascending.                                                     */
int sn_sample_pdf(const float* z_vals, const float* weights, const float* u, long n_rays, int n_samples,
                  int n_importance, float* z_fine, float* z_merged, void* stream);

/* ---- models/rendering.py:15-61  sample_pdf(bins, weights, N_importance, det, eps) exactly as the reference exposes
 * it: bins (n_rays, n_bins+1), weights (n_rays, n_bins) -> samples (n_rays, n_importance); u as above; eps > 0 (the
 * reference default 1e-5 is what render_rays uses, rendering.py:311).                                          */
int sn_sample_pdf_bins(const float* bins, const float* weights, const float* u, long n_rays, int n_bins,
                       int n_importance, float eps, float* samples, void* stream);

/* ==== "next" rows: the steps immediately before / after the hot path ========================== */

/* ---- datasets/ray_utils.py:86-133 (get_ray_directions + get_rays) + the [o, d, near, far] packing of the datasets
 * (e.g. blender_ray_patch_1image_rot3d.py:201-211; strided patches :487-498): rays generated on the GPU.
 * c2w: 12 floats (3x4 row-major, DEVICE).  Pixel (x0 + ix*stride_x, y0 + iy*stride_y), ix < patch_w, iy < patch_h,
 * written row-major over (iy, ix) into rays (patch_w*patch_h, 8).  Full frame = (0, 0, 1, 1, W, H).             */
int sn_generate_rays(const float* c2w, int H, int W, float focal, float near, float far, int x0, int y0, int stride_x,
                     int stride_y, int patch_w, int patch_h, float* rays, void* stream);

/* ---- backward of sn_generate_rays with respect to c2w (datasets/ray_utils.py:109, :112: rays_d = directions @ c2w[:, :3].T,
 * rays_o = c2w[:, 3]):  g_c2w[a][b] = sum_rays g_rays[r, 3 + a] * dir_cam_r[b]  (b < 3),  g_c2w[a][3] = sum_rays g_rays[r, a], with
 * dir_cam = ((x - W/2) / focal, -(y - H/2) / focal, -1) of the pixel of that row (ray_utils.py:89-91).  g_rays (patch_w * patch_h, 8):
 * the upstream gradient of the rays (columns 6, 7 ignored); window arguments as for sn_generate_rays.  g_c2w: 12 floats (3x4
 * row-major, DEVICE), written.  workspace: sn_generate_rays_backward_workspace_bytes bytes of DEVICE scratch (per-block fp64
 * partial sums, added in a fixed order: deterministic).                                                                */
long sn_generate_rays_backward_workspace_bytes(void);
int sn_generate_rays_backward(const float* g_rays, int H, int W, float focal, int x0, int y0, int stride_x, int stride_y,
                              int patch_w, int patch_h, void* workspace, float* g_c2w, void* stream);

/* ---- sn_generate_rays for the reference's other cameras.  datasets/ray_utils.py:89-91 + :109-114 (blender, llff) or
 * datasets/dtu_proj.py:31-33 + ray_utils.py:109-114 (dtu), then optionally get_ndc_rays (datasets/ray_utils.py:144-162, the call
 * sites llff_ray_patch_1image_proj.py:473-483, :541-545, :676-682), and the [o, d, near, far] packing.
 * Camera direction of pixel (i, j):  convention 0 = ((i - cx) / fx, -(j - cy) / fy, -1);  convention 1 = ((i - cx) / fx, (j - cy) / fy, +1).
 * ndc = 1: every ray goes through the NDC map of sn_ndc_rays with (H, W, ndc_focal, ndc_near) before it is written; ndc = 0: ndc_near
 * is ignored, ndc_focal is still checked (pass fx).  near, far: columns 6, 7 as given (llff with NDC: 0, 1).  c2w, window, rays: as
 * for sn_generate_rays, whose bits (convention 0, fx = fy = focal, cx = W/2, cy = H/2, ndc = 0) reproduces.
 * SN_E_BADARG: convention or ndc not in {0, 1}; fx, fy or ndc_focal not finite or not positive.                              */
int sn_generate_rays_cam(const float* c2w, int H, int W, float fx, float fy, float cx, float cy, int convention, int ndc,
                         float ndc_focal, float ndc_near, float near, float far, int x0, int y0, int stride_x, int stride_y,
                         int patch_w, int patch_h, float* rays, void* stream);

/* ---- backward of sn_generate_rays_cam with respect to c2w: autograd of the lines above.  With ndc = 1 the gradient of each ray first
 * goes back through the NDC map (as sn_ndc_rays_backward, at the world ray recomputed from c2w; no (n, 8) intermediate is written), then
 * the 12 sums of sn_generate_rays_backward with this camera's directions.  c2w: 12 floats (DEVICE), read only when ndc = 1 (may be NULL
 * otherwise).  workspace: sn_generate_rays_backward_workspace_bytes bytes.  Deterministic; with ndc = 0 and the camera of
 * sn_generate_rays, the bits of sn_generate_rays_backward.                                                                   */
int sn_generate_rays_cam_backward(const float* g_rays, const float* c2w, int H, int W, float fx, float fy, float cx, float cy,
                                  int convention, int ndc, float ndc_focal, float ndc_near, int x0, int y0, int stride_x,
                                  int stride_y, int patch_w, int patch_h, void* workspace, float* g_c2w, void* stream);

/* ---- datasets/ray_utils.py:123-164 get_ndc_rays(H, W, focal, near, rays_o, rays_d) over rays that exist already: rays_in (n_rays, 8)
 * [o, d, near, far] in world space -> rays_out (n_rays, 8) in NDC; columns 6, 7 are copied.  Computed op by op in the reference's
 * order, one fp32 rounding per op; -1/(W/(2 focal)) and -1/(H/(2 focal)) are formed in double and cast once, as Python does.  A ray with
 * d_z == 0 gives the reference's inf / NaN.  In place is allowed: rays_out may be rays_in.                                    */
int sn_ndc_rays(const float* rays_in, long n_rays, int H, int W, float focal, float ndc_near, float* rays_out, void* stream);

/* ---- backward of sn_ndc_rays: autograd of datasets/ray_utils.py:145-159 in fp32 with the forward intermediates recomputed from
 * rays_in (the map's INPUT).  g_rays_out (n_rays, 8): gradient of the NDC rays (columns 6, 7 ignored) -> g_rays_in (n_rays, 8): gradient
 * of the world rays, columns 6, 7 zero.  The shifted o_z is only approximately -near: its derivative terms are kept.
 * g_rays_in must not overlap the inputs.                                                                                     */
int sn_ndc_rays_backward(const float* rays_in, const float* g_rays_out, long n_rays, int H, int W, float focal, float ndc_near,
                         float* g_rays_in, void* stream);

/* ---- the camera entries with the INTRINSICS IN DEVICE MEMORY and their gradients (additive within ABI 5): a focal length that is
 * being learnt lives in a device tensor; these entries never read it back, so they neither synchronise nor break a stream capture.
 * intr: 4 floats (DEVICE) fx, fy, cx, cy;  with ndc = 1 the NDC map's focal length is intr[0] (ndc_focal = fx above).  The kernels are
 * those of the entries above with the camera filled in on the device; -1/(W/(2 focal)), -1/(H/(2 focal)) are formed there in fp64
 * with one cast, as on the host: for equal fp32 values sn_generate_rays_cam_dev writes the bits of sn_generate_rays_cam and
 * sn_ndc_rays_dev those of sn_ndc_rays (in place allowed).  Pointers, H, W, the window, convention and ndc are refused on the host as
 * above.  The VALUES of the intrinsics are NOT checked (that would need a sync): a focal length that is zero, negative or not finite
 * gives what IEEE arithmetic gives -- inf / NaN rays and gradients, as the reference's torch ops would -- and no fault.           */
int sn_generate_rays_cam_dev(const float* c2w, const float* intr, int H, int W, int convention, int ndc, float ndc_near, float near,
                             float far, int x0, int y0, int stride_x, int stride_y, int patch_w, int patch_h, float* rays,
                             void* stream);

/* ---- backward of sn_generate_rays_cam_dev with respect to c2w AND the intrinsics.  g_c2w (12 floats) or g_intr (4 floats: dL/dfx,
 * dL/dfy, dL/dcx, dL/dcy) may be NULL and is then not written; both NULL: SN_E_BADARG.  c2w is always read.  Per ray, with c the
 * camera direction, gd the gradient of the world direction (after the NDC adjoint with ndc = 1), gc = c2w[:, :3]^T gd and s = -1 / +1
 * for convention 0 / 1:   g_fx += gc0 (-c0 / fx),  g_cx += gc0 (-1 / fx),  g_fy += gc1 (-c1 / fy),  g_cy += gc1 (-s / fy);
 * with ndc = 1, from the gradient (go', gd') of the map's output and its quotients:  g_ax += go'0 ox_oz + gd'0 (u - ox_oz),
 * g_ay += go'1 oy_oz + gd'1 (v - oy_oz),  and g_intr[0] += g_ax (-2 / W) + g_ay (-2 / H).  Per-ray terms from the fp32 quantities of the
 * forward, products and sums in fp64, per-block partials added in index order: deterministic, no atomics.  g_c2w has the bits of
 * sn_generate_rays_cam_backward.  An empty window writes zeros.  workspace: sn_camera_backward_workspace_bytes bytes (DEVICE).      */
long sn_camera_backward_workspace_bytes(void);
int sn_generate_rays_cam_dev_backward(const float* g_rays, const float* c2w, const float* intr, int H, int W, int convention, int ndc,
                                      float ndc_near, int x0, int y0, int stride_x, int stride_y, int patch_w, int patch_h,
                                      void* workspace, float* g_c2w, float* g_intr, void* stream);

/* ---- sn_ndc_rays / sn_ndc_rays_backward with the focal length in DEVICE memory (focal: 1 float).  The backward writes g_rays_in with
 * the bits of sn_ndc_rays_backward and g_focal (1 float) = g_ax (-2 / W) + g_ay (-2 / H) from the sums above (zero for n_rays = 0);
 * workspace: sn_camera_backward_workspace_bytes bytes.  The value of focal is not checked, as above.                             */
int sn_ndc_rays_dev(const float* rays_in, long n_rays, int H, int W, const float* focal, float ndc_near, float* rays_out,
                    void* stream);
int sn_ndc_rays_dev_backward(const float* rays_in, const float* g_rays_out, long n_rays, int H, int W, const float* focal,
                             float ndc_near, void* workspace, float* g_rays_in, float* g_focal, void* stream);

/* ---- utils/__init__.py:19-21 (torch.optim.Adam, eps=1e-8) over one flat fp32 buffer (the all-reduce buffer).
 * step = 1-based iteration count (bias correction).                                                             */
int sn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int step, void* stream);

/* ---- the reference's other optimisers (opt.py --optimizer {sgd, radam, ranger}; utils/__init__.py:16-27) over the same flat fp32
 * buffers, one launch each, in place (additive within ABI 5).  n >= 0 elements (n = 0: nothing is launched, returns 0); buffers are
 * DEVICE fp32 of n elements and must not overlap.  The scalars are doubles the CALLER computes on the host (from its own step
 * counter: nothing is read back from the device); each is rounded to fp32 once, as torch rounds a Python scalar, and the arithmetic
 * is fp32 with one rounding per operation.
 *
 * sn_sgd_step -- torch.optim.SGD, dampening 0, no Nesterov:
 *   g += weight_decay p (when != 0) ; buf = momentum buf + g ; p -= lr buf.  A zero-initialised buf reproduces torch's first step
 *   (buf = g).  momentum == 0: p -= lr g, momentum_buf is not touched and may be NULL.
 *
 * sn_radam_step -- the element-wise part of utils/optimizers.py:62-104, in that order:
 *   v = v beta2 + (1 - beta2) g g ; m = m beta1 + (1 - beta1) g                    (always)
 *   p -= decay p (when decay != 0; decay = weight_decay lr: decoupled, applied to the parameter)
 *   p -= step_coeff m / (sqrt(v) + eps) when rectified != 0, else p -= step_coeff m         (step_coeff = step_size lr)
 *   step_coeff < 0: no parameter update this step and no decay (degenerated_to_sgd=False below the N_sma threshold, :86-87, 99).
 *
 * sn_ranger_step -- utils/optimizers.py:393-437: the same moments and update with the decay applied on every step (:416-418;
 *   step_coeff < 0 is refused), then, when sync != 0, the lookahead of :431-437 in the same launch:
 *   slow += alpha (p - slow) ; p = slow.  slow (n) is read and written only when sync != 0, but must always be given.            */
int sn_sgd_step(float* params, const float* grads, float* momentum_buf, long n, double lr, double momentum, double weight_decay,
                void* stream);
int sn_radam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, double beta1, double beta2, double eps,
                  double decay, double step_coeff, int rectified, void* stream);
int sn_ranger_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, double beta1, double beta2, double eps,
                   double decay, double step_coeff, int rectified, float* slow, double alpha, int sync, void* stream);

/* ---- losses on the rendered rays, forward + gradients in two launches: MSELoss (losses.py:12-22: nn.MSELoss 'mean' of
 * rgb_coarse and rgb_fine against the targets), SL1Loss (models/sinnerf.py:32-42: nn.SmoothL1Loss 'mean', beta 1, of
 * depth_coarse and depth_fine -- call sites :310-319) and psnr (metrics.py:5-15).
 *   rgb_* (n,3), depth_* (n), rgb_gt (n,3), depth_gt (n): DEVICE fp32; any prediction and either target may be NULL
 *   (its terms are then 0 and its gradient is not written).
 *   mask_mode 0: every depth element counts (useMask=False); 1: depth_gt > 0 (mask=None, useMask=True); 2: mask (n) uint8.
 *   out[8] = mse_coarse, mse_fine, sl1_coarse, sl1_fine, total = w_rgb (mse_c + mse_f) + w_depth (sl1_c + sl1_f),
 *            psnr_coarse, psnr_fine, number of depth elements counted.
 *   g_*: gradients of `total` w.r.t. the matching prediction (NULL = not wanted).
 *   workspace: sn_render_loss_workspace_bytes() bytes of DEVICE scratch (per-block partial sums; deterministic order). */
long sn_render_loss_workspace_bytes(void);
int sn_render_loss(const float* rgb_coarse, const float* rgb_fine, const float* depth_coarse, const float* depth_fine,
                   const float* rgb_gt, const float* depth_gt, const unsigned char* mask, int mask_mode, long n,
                   float w_rgb, float w_depth, float* g_rgb_coarse, float* g_rgb_fine, float* g_depth_coarse,
                   float* g_depth_fine, void* workspace, float* out, void* stream);

/* ---- losses on the rendered PATCHES, forward + gradients in two launches (additive within ABI 5): losses.py:94-109 L2_SSIM_Loss --
 * nn.MSELoss 'mean' of coarse and of fine against the target, plus w_ssim x kornia 0.6.3 ssim_loss of fine against the target:
 *   g[k] = exp(-(k - window/2)^2 / (2 1.5^2)) normalised to sum 1; F = per-channel correlation with g (x) g after reflect padding by
 *   window/2 (the edge pixel is not repeated); mu1 = F(a), mu2 = F(b), s11 = F(a a) - mu1^2, s22 = F(b b) - mu2^2, s12 = F(a b) - mu1 mu2;
 *   ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2) + 1e-12), C1 = 0.01^2, C2 = 0.03^2;
 *   ssim_loss = mean over B C H W of clamp((1 - ssim) / 2, 0, 1); the clamp passes gradient strictly inside (0, 1).
 *   coarse, fine, target: DEVICE fp32 (B, H, W, C), CHANNEL-LAST -- the (B H W, C) rows of a render, or its (B H W) depths with C = 1.
 *   coarse or fine may be NULL (its term is 0), not both; use_ssim needs fine.
 *   use_ssim = 0: the MSE pair alone, any C (losses.py:12-22 on a patch); window is ignored.
 *   out[4] = mse_coarse, mse_fine, ssim_loss, total = w_mse (mse_coarse + mse_fine) + w_ssim ssim_loss.
 *   g_coarse, g_fine: gradients of `total`, channel-last (NULL = not wanted).  The target receives none.
 *   workspace: the bytes the query returns for the same (B, H, W, C, use_ssim), DEVICE scratch.  Results are deterministic.
 * SN_E_BADARG: a null required pointer; B, H, W or C <= 0; with use_ssim an even or non-positive window or C not in {1, 3}.
 * SN_E_BADSHAPE: with use_ssim, H <= window/2 or W <= window/2.  SN_E_UNSUPPORTED: window > SN_PATCH_LOSS_MAX_WINDOW.
 * SN_E_TOOLARGE: 2^31 elements or more.                                                                                      */
#define SN_PATCH_LOSS_MAX_WINDOW 31
long sn_patch_loss_workspace_bytes(int B, int H, int W, int C, int use_ssim);
int sn_patch_loss(const float* coarse, const float* fine, const float* target, int B, int H, int W, int C, int use_ssim, int window,
                  float w_mse, float w_ssim, float* g_coarse, float* g_fine, void* workspace, float* out, void* stream);

/* ---- kornia inverse_depth_smoothness_loss(idepth, image) (models/sinnerf.py:370-373, 395-398), forward + gradients in two launches:
 *   dx(t) = t[.., :, :-1] - t[.., :, 1:], dy alike along H; wx = exp(-mean_c |dx(image)|), wy alike;
 *   out[0] = mean |dx(idepth) wx| + mean |dy(idepth) wy|.
 *   idepth (B, H, W), image (B, H, W, C) channel-last: DEVICE fp32.  g_idepth, g_image: gradients of out[0] in the same layouts (NULL =
 *   not wanted); |.| has derivative sign with sign(0) = 0.  workspace: the bytes the query returns.
 * SN_E_BADARG: a null required pointer; B, H, W or C <= 0.  SN_E_BADSHAPE: H < 2 or W < 2.  SN_E_TOOLARGE: 2^31 elements or more.   */
long sn_depth_smoothness_workspace_bytes(void);
int sn_depth_smoothness(const float* idepth, const float* image, int B, int H, int W, int C, float* g_idepth, float* g_image,
                        void* workspace, float* out, void* stream);

/* ---- regularisers on the distribution of the compositing weights along a ray, forward + gradients in two launches (additive within
 * ABI 5): the distortion loss of Mip-NeRF 360 (eq. 15) and the ray entropy of InfoNeRF (eqs. 5-7).  Per ray of S = n_samples samples,
 * weights w_i, depths z_i (ascending, ties allowed), near = rays[r, 6], far = rays[r, 7]:
 *   inv  = far > near ? 1 / (far - near) : 0;  s_i = (z_i - near) inv;
 *   m_i  = (s_i + s_{i+1}) / 2 for i < S - 1, m_{S-1} = s_{S-1};  d_i = s_{i+1} - s_i for i < S - 1, d_{S-1} = 0 (the compositor's
 *          1e10 last delta is not a length);
 *   dist = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i;
 *   o = sum_i w_i, q = o + 1e-10, p_i = w_i / q, H = -sum_i p_i log(p_i + 1e-10); mask = o > ent_threshold (a constant for the
 *   gradient); ent = mask ? H : 0.
 *   Both are means over ALL n_rays rays (the entropy as mean(mask H), not a mean over the masked rays);
 *   total = w_dist mean(dist) + w_ent mean(ent).
 *   weights, z_vals (n_rays, n_samples), rays (n_rays, 8): DEVICE fp32.  z_vals, near and far are data: no gradient.
 *   g_weights (n_rays, n_samples): d total / d weights = (w_dist ddist/dw + w_ent mask dH/dw) / n_rays, written, not accumulated; NULL =
 *   not wanted.  per_ray (n_rays, 2) = (dist, ent) of each ray; NULL = not wanted.
 *   out[4] = mean dist, mean ent, total, number of rays with the mask set.
 *   workspace: the bytes the query returns for n_rays, DEVICE scratch.  fp64 arithmetic on the fp32 inputs, one rounding per output,
 *   sums in a fixed order without atomics: two calls give the same bits.  No host read-back, no allocation: capturable.
 * SN_E_BADARG: a null required pointer.  SN_E_BADSHAPE: n_samples outside 1..1024.  SN_E_TOOLARGE: more than 2^33 - 4 rays.
 * n_rays <= 0 launches nothing, sets out to {0, 0, 0, 0} on the stream and returns 0.                                              */
long sn_ray_regularizers_workspace_bytes(long n_rays);
int sn_ray_regularizers(const float* weights, const float* z_vals, const float* rays, long n_rays, int n_samples, float w_dist,
                        float w_ent, float ent_threshold, float* g_weights, float* per_ray, void* workspace, float* out, void* stream);

/* ---- the unseen-view reprojection loss, forward + gradients in two launches (additive within ABI 5): the INVERSE warp of a render into
 * the reference camera -- the view-synthesis loss of SfMLearner / MonoDepth2 with an occlusion test against the reference depth, and a
 * free-space term on rendered surfaces in front of what the reference camera saw.  All pointers are DEVICE pointers, ref_proj included.
 *   rays (n, 8): o = rays[:, 0:3], d = rays[:, 3:6], in WORLD space (not NDC); depth (n): the rendered depth t along each ray;
 *   rgb (n, C) channel-last, C in 1..4; opacity (n) or NULL; ref_image (H, W, C) channel-last, ref_depth (H, W);
 *   ref_proj[16]: fp64, row-major, the [K E[:3]; 0 0 0 1] matrix of the reference camera (as sn_forward_warp takes it).
 *   Integer pixel coordinates are sample positions (sn_forward_warp un-projects source pixel (x, y) the same way).
 * All in fp64 on the fp32 inputs; every mask is a constant for the gradient.  Per pixel i:
 *   X = o + t d;  q = P[:3,:3] X + P[:3,3];  z = q2, u = q0 / z, v = q1 / z;
 *   G (geometrically valid): t finite and t > 0;  z >= z_min;  opacity NULL or opacity_i > opacity_threshold;  0 <= u <= W - 1 and
 *     0 <= v <= H - 1;  the four corner depths all > 0 (a zero depth is background).  Every comparison is false for NaN.
 *   x0 = min(floor(u), W - 2), y0 = min(floor(v), H - 2), fx = u - x0, fy = v - y0 (so u = W - 1 is inside, with fx = 1);
 *   bilinear samples with s00 = s[y0, x0], s10 = s[y0, x0 + 1], s01 = s[y0 + 1, x0], s11 = s[y0 + 1, x0 + 1]:
 *     s = (1 - fy)((1 - fx) s00 + fx s10) + fy((1 - fx) s01 + fx s11);  D from ref_depth, c_c from ref_image;
 *   r = (z - D) / D;  V (visible) = G and |r| <= occ_tol;
 *   photo_i = (1/C) sum_c sqrt((rgb_ic - c_c)^2 + charb_eps^2);  free_i = max(0, -r - occ_tol);  front_i = free_i > 0;
 *   n_vis = sum V, n_geo = sum G, n_front = sum front;
 *   photo = n_vis ? sum_V photo_i / n_vis : 0;  free = n_geo ? sum_G free_i / n_geo : 0;  total = w_photo photo + w_free free;
 *   out[6] = photo, free, total, n_vis, n_geo, n_front.
 * Gradients of `total`, through the sampling coordinates (the spatial-transformer derivative):
 *   a = P[:3,:3] d;  z_t = a2, u_t = (a0 - u a2) / z, v_t = (a1 - v a2) / z;
 *   slopes ds/du = (1 - fy)(s10 - s00) + fy (s11 - s01), ds/dv = (1 - fx)(s01 - s00) + fx (s11 - s10);
 *   s_ic = (rgb_ic - c_c) / sqrt((rgb_ic - c_c)^2 + charb_eps^2);
 *   g_rgb_ic = w_photo V_i s_ic / (n_vis C);
 *   g_depth_i = -(w_photo V_i / (n_vis C)) sum_c s_ic (dc_c/du u_t + dc_c/dv v_t) + (w_free G_i front_i / n_geo) (-r_t),
 *   r_t = a2 / D - z (dD/du u_t + dD/dv v_t) / D^2.
 *   g_depth (n), g_rgb (n, C): WRITTEN, not accumulated, exactly 0 wherever the mask is off (no NaN leaks from an invalid pixel).
 *   per_pixel (n, 2) = (V ? photo_i : 0, G ? free_i : 0).  flags (n) uint8: bit 0 = G, bit 1 = V, bit 2 = front.
 *   Any of g_depth, g_rgb, per_pixel, flags may be NULL.  The rays, the reference frame and ref_proj receive no gradient.
 *   workspace: the bytes the query returns for n, DEVICE scratch.  One rounding to fp32 per output, sums in a fixed order without
 *   atomics: two calls give the same bits.  No host read-back, no allocation: capturable.
 * SN_E_BADARG: a null required pointer; H < 2 or W < 2; C outside 1..4.  SN_E_TOOLARGE: n or H W C >= 2^31.
 * n <= 0 launches nothing, sets out to zeros on the stream and returns 0.                                                          */
long sn_reproject_loss_workspace_bytes(long n);
int sn_reproject_loss(const float* rays, const float* depth, const float* rgb, const float* opacity, long n, int C,
                      const float* ref_image, const float* ref_depth, int H, int W, const double* ref_proj, float occ_tol,
                      float charb_eps, float z_min, float opacity_threshold, float w_photo, float w_free, float* g_depth, float* g_rgb,
                      float* per_pixel, unsigned char* flags, void* workspace, float* out, void* stream);

/* ---- the forward warp of the reference view and its depth into the unseen view (additive within ABI 5): project_with_depth +
 * forward_warp of datasets/blender_ray_patch_1image_rot3d.py:103-150 (called per training sample, :481-484),
 * blender_ray_patch_1image_proj.py:93-138 (with depth_mask, :135-137), llff_ray_patch_1image_proj.py:117-166 (painter's loop :161-165)
 * and warp_img_proj_numpy of dtu_proj.py:236-273 (loop :266-271), as one rule.  All pointers are DEVICE pointers.
 *   ref_depth (H, W) fp32; data (H, W, C) fp32 CHANNEL-LAST, may be NULL (C is then ignored and out_new is not written).
 *   ref_proj[16], src_proj[16]: fp64, row-major 4x4, the [K E[:3]; 0 0 0 1] matrices dtu_proj.py passes and the others imply.
 *   In fp64 on the device: M = (src_proj ref_proj^-1)[:3, :] (Gauss-Jordan, once); for source pixel (x, y) of depth d
 *   p = M (x d, y d, d, 1); depth_src = (float)p2; xs = p0 / (p2 + eps), ys = p1 / (p2 + eps)  (eps: 1e-9 at llff :136, 0 at dtu);
 *   target tx = clamp(floor(xs), 0, W - 1), ty = clamp(floor(ys), 0, H - 1), clamped in floating point before the integer conversion,
 *   so +-inf ends on a border.  A NaN xs or ys DROPS the source pixel: the reference casts NaN to int64, which is undefined
 *   (rot3d :145 "be careful with nan").  Zero-depth source pixels take part as in the reference (they share one target).
 *   mode 0: the LAST source pixel in raster order wins a target (NumPy's fancy-index assignment with duplicates: the blender files).
 *   mode 1: the smallest depth_src (as fp32) wins, ties to the lowest raster index: the painter's loop of llff and dtu -- except
 *   where a depth_src is exactly 0.0, which that loop reads as "empty" and overwrites.
 *   The scatter always covers the whole frame.  The window (x0, y0, stride_x, stride_y, out_w, out_h), as in sn_generate_rays (full
 *   frame = (0, 0, 1, 1, W, H)), selects what is written, row-major over (iy, ix); any output may be NULL:
 *     out_new (out_h out_w, C) the winner's data row bit for bit, zeros where nothing landed;  new_depth (out_h out_w) its depth_src, 0
 *     where nothing landed;  mask (out_h out_w) uint8, 1 where a pixel landed (depth_mask);  winner (out_h out_w) int32 source raster
 *     index or -1.
 *   workspace: the bytes the query returns for (H, W); it need not be initialised (the keys are cleared on the stream).  Results are
 *   deterministic: the same bits on every call.
 * SN_E_BADARG: a null required pointer; H, W, stride_x, stride_y, out_w or out_h <= 0; a window that leaves the frame; mode not in
 * {0, 1}; data given with C <= 0.  SN_E_TOOLARGE: H W >= 2^31.                                                               */
long sn_forward_warp_workspace_bytes(int H, int W);
int sn_forward_warp(const float* ref_depth, const float* data, int H, int W, int C, const double* ref_proj, const double* src_proj,
                    double eps, int mode, int x0, int y0, int stride_x, int stride_y, int out_w, int out_h, float* out_new,
                    float* new_depth, unsigned char* mask, int* winner, void* workspace, void* stream);

/* ---- np.random.choice(len(proj_depths_full), num) over rays_full[depth_mask] (blender_ray_patch_1image_proj.py:390-394, :472-478)
 * without the boolean compaction: with N = the number of non-zero elements of mask (n) uint8, idx[j] (int32) = the raster index of
 * the min(floor((double)u[j] N), N - 1)-th of them in raster order, for u (m) fp32 in [0, 1) (a u outside, or NaN, is clamped to the
 * first / last); N = 0 gives idx = -1 everywhere.  n_landed (one int32, may be NULL) receives N.  All DEVICE pointers; m may be 0.
 * Block sums, their scan, a search over blocks and a ballot walk inside one: integer sums without atomics, deterministic.
 * workspace: the bytes the query returns for n.
 * SN_E_BADARG: a null required pointer, n <= 0, m < 0.  SN_E_TOOLARGE: n or m >= 2^31.                                          */
long sn_select_landed_workspace_bytes(long n);
int sn_select_landed(const unsigned char* mask, long n, const float* u, long m, int* idx, int* n_landed, void* workspace,
                     void* stream);

/* ---- the one-image training sampler (additive within ABI 5; sinnerf_amd/sampler.py): the device form of the two rejection loops of
 * datasets/blender_ray_patch_1image_rot3d.py:451-460 and :486-499, and of the strided slices of :456-457, :491-497 and :523-528.
 *
 * A loop that redraws a uniform window origin until the window has content accepts an origin uniform over the origins WITH content:
 * that is "the floor(u N)-th set element" (sn_select_landed) of the map sn_valid_windows writes.
 *   mask (H, W) uint8, non-zero = set.  A window at origin (x0, y0) -- x the column -- covers the pixels (y0 + j stride_y,
 *   x0 + i stride_x), 0 <= j < patch_h, 0 <= i < patch_w.  Candidates: 0 <= x0 < nx, 0 <= y0 < ny.
 *   valid (ny, nx) uint8: 1 where any pixel of the window is set, else 0.  n_valid (one int32, may be NULL) receives the sum of valid.
 *   Two passes, rows then columns (patch_w + patch_h reads per origin), integer sums: the same bits on every call.
 *   workspace: the bytes the query returns for (H, nx); it need not be initialised.
 * SN_E_BADARG: a null required pointer; H, W, a stride, a patch size, nx or ny <= 0; a candidate window that leaves the frame, that is
 * nx > W - (patch_w - 1) stride_x or ny > H - (patch_h - 1) stride_y.  SN_E_TOOLARGE: H W >= 2^31.                                 */
long sn_valid_windows_workspace_bytes(int H, int nx);
int sn_valid_windows(const unsigned char* mask, int H, int W, int stride_x, int stride_y, int patch_w, int patch_h, int nx, int ny,
                     unsigned char* valid, int* n_valid, void* workspace, void* stream);

/* One strided window out of n_src (1..SN_GATHER_MAX_SOURCES) full-frame CHANNEL-LAST arrays of 32-bit words, in one launch.
 *   src[k] (H, W, channels[k]) and dst[k] are DEVICE pointers; the arrays src, dst and channels themselves are HOST arrays of n_src
 *   entries, read during the call and handed to the kernel by value.  dst[k] is written as (patch_h, patch_w, channels[k]), or planar
 *   (channels[k], patch_h, patch_w) where bit k of planar_mask is set; it must not overlap a source.  Words are copied bit for bit.
 *   origin: two int32 in DEVICE memory, (x0, y0), read by the kernel -- typically formed from the index sn_select_landed wrote.  Each is
 *   clamped into [0, W - (patch_w - 1) stride_x) resp. [0, H - (patch_h - 1) stride_y), so that an origin of -1 (nothing valid) reads the
 *   window at 0 and no value of the two words can make the kernel read outside a source.
 * SN_E_BADARG: a null pointer (an entry of src or dst included); n_src outside 1..8; a bit of planar_mask at or above n_src; H, W, a
 * stride, a patch size or a channel count <= 0; a window that fits at no origin.  SN_E_TOOLARGE: H W channels[k] >= 2^31.      */
#define SN_GATHER_MAX_SOURCES 8
int sn_gather_windows(const void* const* src, void* const* dst, const int* channels, int n_src, unsigned planar_mask, int H, int W,
                      const int* origin, int stride_x, int stride_y, int patch_w, int patch_h, void* stream);

#ifdef __cplusplus
}
#endif
#endif
