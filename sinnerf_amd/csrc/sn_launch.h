// sn_launch.h -- host-side launch hygiene shared by the launchers: device properties and per-kernel attributes are queried /
// set ONCE per (device, kernel) instead of on every launch (hipDeviceGetAttribute + hipFuncSetAttribute cost a few
// microseconds each -- invisible next to a 170 ms frame, not next to the ~1 ms launches of a mixed-precision training step),
// and nothing here synchronises or allocates, so every launcher stays capturable in a HIP graph.
//
// It also holds the ONE set of prototypes of every host function that crosses a translation unit (the *_launch / *_impl functions
// sn_api.hip and sn_dw.hip call): the defining files include this header too, so a definition whose parameter list differs from the
// declaration its callers see is a compile error (C linkage cannot be overloaded) instead of a link that shifts arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include "../../include/sinnerf_hip.h"
#include "sn_device.h"

namespace snh {

constexpr int MAX_DEVICES = 64;

inline int current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return -1;
  return dev;
}

// compute units of the current device (persistent kernels launch one workgroup per CU)
inline int cu_count() {
  static int cached[MAX_DEVICES];              // 0 = not queried yet (benign race: every thread writes the same value)
  const int dev = current_device();
  if (dev < 0) return 256;
  int v = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
  if (v == 0) {
    v = 256;
    (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    __atomic_store_n(&cached[dev], v, __ATOMIC_RELAXED);
  }
  return v;
}

// grid of a persistent kernel that walks `tiles` point tiles: one workgroup per CU, fewer when there are fewer tiles
inline unsigned persistent_grid(long tiles) {
  const int n_cu = cu_count();
  return (unsigned)(tiles < n_cu ? tiles : n_cu);
}

// grid of a one-wave-per-ray kernel: blocks of 256 threads = four rays each.  Returns 0, or SN_E_TOOLARGE beyond what a grid holds.
inline long ray_blocks(long n_rays) { return (n_rays + 3) / 4; }
inline int ray_grid(long n_rays, dim3* grid) {
  const long blocks = ray_blocks(n_rays);
  if (blocks > 0x7fffffffL) return SN_E_TOOLARGE;
  *grid = dim3((unsigned)blocks);
  return 0;
}

// ... and its samples per lane C = ceil(n_samples / 64): lane l owns the samples [l C, (l + 1) C).  0: outside the 1..16 the kernels
// are instantiated for (the entry names the error).  for_samples_per_lane calls f(std::integral_constant<int, C>) for that C.
inline int samples_per_lane(int n_samples) {
  const int C = (n_samples + 63) / 64;
  return C >= 1 && C <= 16 ? C : 0;
}
template <typename F>
inline void for_samples_per_lane(int C, F&& f) {
  switch (C) {
#define SN_C_(CC) case CC: f(std::integral_constant<int, CC>{}); break;
    SN_C_(1) SN_C_(2) SN_C_(3) SN_C_(4) SN_C_(5) SN_C_(6) SN_C_(7) SN_C_(8)
    SN_C_(9) SN_C_(10) SN_C_(11) SN_C_(12) SN_C_(13) SN_C_(14) SN_C_(15) SN_C_(16)
#undef SN_C_
  }
}

// blocks of 256 threads of a grid-stride kernel over n > 0 elements, at most cap; the _min1 form for a launch that must run on
// empty input too (its finisher still writes zeros)
inline unsigned stride_grid(long n, long cap) {
  const long blocks = (n + 255) / 256;
  return (unsigned)(blocks > cap ? cap : blocks);
}
inline unsigned stride_grid_min1(long n, long cap) { return n > 0 ? stride_grid(n, cap) : 1u; }

// Kernels that deal their work units dynamically (sn_mlp_fwd_f32g.hip) draw tickets from one word of a per-device array of UNIT_WORDS
// words that the kernel's translation unit owns.  unit_word(stream) = the index of the stream's word on the current device: launches on
// one stream run one after the other and share a word (each zeroes it on the stream first), two streams never share one.  The map only
// grows (a destroyed stream's handle, when the runtime hands it out again, keeps its word); -1 once UNIT_WORDS streams have been seen.
constexpr int UNIT_WORDS = 1024;
inline int unit_word(hipStream_t stream) {
  static std::mutex mu;
  static std::unordered_map<hipStream_t, int> of[MAX_DEVICES];
  const int dev = current_device();
  if (dev < 0) return -1;
  std::lock_guard<std::mutex> lock(mu);
  auto it = of[dev].find(stream);
  if (it != of[dev].end()) return it->second;
  const int w = (int)of[dev].size();
  if (w >= UNIT_WORDS) return -1;
  of[dev].emplace(stream, w);
  return w;
}

// SN_DTYPE_EMB_BF16 (emb stored as bf16 in K-slot order) is refused unless the arithmetic is SN_DTYPE_BF16_STATE and the generated
// narrow weight-gradient kernel -- the only reader of that form -- will run: a caller that asks sn_weight_grads_workspace_bytes first
// (sinnerf_amd/autograd.py does) never stores a bf16 emb the backward cannot read.
#ifndef SN_DW_NARROW_ASM
#define SN_DW_NARROW_ASM 1      // bf16-state narrow problems on the generated instruction streams (0: comparison build)
#endif
// SINNERF_DW_NARROW_COMPILER=1 in the environment keeps the compiler-scheduled narrow kernel (A/B runs; read once)
inline bool narrow_compiler_scheduled() {
  static const bool v = [] { const char* e = getenv("SINNERF_DW_NARROW_COMPILER"); return e != nullptr && e[0] == '1'; }();
  return v;
}
inline bool emb16_refused(int base_dtype, int emb16) {
  return emb16 && (base_dtype != SN_DTYPE_BF16_STATE || !SN_DW_NARROW_ASM || narrow_compiler_scheduled());
}

}  // namespace snh

// Raise the dynamic-LDS limit of kernel KFN_ to LDS_ bytes once per device.  Expands to a block with its own static
// high-water marks, so every call site (= every kernel instantiation) is tracked separately.  `return`s the hipError_t
// as int from the enclosing launcher on failure.
#define SN_ENSURE_DYN_LDS(KFN_, LDS_)                                                                               \
  do {                                                                                                              \
    static int sn_lds_set_[snh::MAX_DEVICES];                                                                       \
    const int sn_dev_ = snh::current_device();                                                                      \
    if (sn_dev_ < 0 || __atomic_load_n(&sn_lds_set_[sn_dev_], __ATOMIC_RELAXED) < (int)(LDS_)) {                    \
      hipError_t sn_e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(KFN_),                                   \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_));              \
      if (sn_e_ != hipSuccess) return (int)sn_e_;                                                                   \
      if (sn_dev_ >= 0) __atomic_store_n(&sn_lds_set_[sn_dev_], (int)(LDS_), __ATOMIC_RELAXED);                     \
    }                                                                                                               \
  } while (0)

// ---------------------------------------------------------------------------------------------------------------------------------
// prototypes (see the top of the file).  SN_DECLARE_HEADS / SN_DECLARE_HEADS_F16 are defined next to SN_LAUNCH_NAME in sn_device.h.
namespace snd { struct Plan; }                  // sn_dw_common.h
extern "C" {
#define SN_FWD_PARAMS_                                                                                                              \
  const void* blob, const float* in0, const float* in1, long n_points, int s_or_ld, int sigma_only, int input_mode, float* out,    \
      float* acts, float* emb, long slot_rows
#define SN_CHAIN_PARAMS_                                                                                                            \
  const void* bblob, const float* acts, const float* out_raw, const float* g_raw, long n_points, long slot_rows, float* G, float* g_out
#define SN_RAYS_PARAMS_ const void* blob, const float* rays, const float* z_vals, long n_points, int n_samples, float* out
// forward: (rays, z_vals) or pre-embedded rows, inference and (acts != nullptr) training
SN_DECLARE_HEADS(sn_mlp_forward_f32, (SN_FWD_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_forward_f32g, (SN_FWD_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_forward_f32g_store, (SN_FWD_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_forward_bf16x3, (SN_FWD_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS_F16(sn_mlp_forward_bf16, (SN_FWD_PARAMS_, int state_bf16, hipStream_t stream));
// ... the hand-scheduled / generated kernels: (rays, z_vals) only
SN_DECLARE_HEADS_F16(sn_mlp_forward_bf16_v3, (SN_RAYS_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_forward_bf16_t, (SN_RAYS_PARAMS_, float* acts, float* emb, long slot_rows, int emb16, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_forward_bf16x3_t, (SN_RAYS_PARAMS_, float* acts, float* emb, long slot_rows, hipStream_t stream));
// backward chain
SN_DECLARE_HEADS(sn_mlp_backward_chain_f32, (SN_CHAIN_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_backward_chain_f32g, (SN_CHAIN_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_backward_chain_bf16, (SN_CHAIN_PARAMS_, int state_bf16, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_backward_chain_bf16_t, (SN_CHAIN_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_backward_chain_bf16x3, (SN_CHAIN_PARAMS_, hipStream_t stream));
SN_DECLARE_HEADS(sn_mlp_backward_chain_bf16x3_t, (SN_CHAIN_PARAMS_, hipStream_t stream));
#undef SN_FWD_PARAMS_
#undef SN_CHAIN_PARAMS_
#undef SN_RAYS_PARAMS_
// weight gradients (sn_dw.hip and the generated kernels it launches)
int sn_dw_launch(const void* tasks, int n_tasks, hipStream_t stream);
long sn_weight_grads_workspace_bytes_impl(long slot_rows, int dtype, int emb16);
int sn_weight_grads_plan_impl(long slot_rows, int dtype, int emb16, int* out, int max_probs);
int sn_weight_grads_launch(const void* acts, const float* emb, const void* G, long slot_rows, int dtype, int emb16, void* workspace,
                           float* const* grads, int accumulate, hipStream_t stream);
int sn_dw_f32_asm_launch(const snd::Plan* plan_host, hipStream_t stream);             // sn_dw_f32.hip
int sn_dw_bf16_asm_launch(const snd::Plan* plan_host, hipStream_t stream);            // sn_dw_bf16.hip
int sn_dw_narrow_bf16_asm_launch(const snd::Plan* plan_host, hipStream_t stream);     // sn_dw_narrow_bf16.hip
// per-ray stages (sn_render.hip)
int sn_sample_coarse_launch(const float* rays, long n_rays, int n_samples, int use_disp, float perturb,
                            const float* perturb_rand, float* z_out, hipStream_t stream);
int sn_composite_forward_launch(const float* raw, int has_rgb, const float* z_vals, const float* rays,
                                const float* noise, float noise_std, long n_rays, int n_samples, int white_back,
                                float* rgb, float* depth, float* weights, hipStream_t stream);
int sn_composite_backward_launch(const float* raw, const float* z_vals, const float* rays, const float* noise,
                                 float noise_std, long n_rays, int n_samples, int white_back, const float* g_rgb,
                                 const float* g_depth, const float* g_w, float* g_raw, hipStream_t stream);
int sn_composite_backward_rays_launch(const float* raw, const float* z_vals, const float* rays, const float* noise,
                                      float noise_std, long n_rays, int n_samples, int white_back, const float* g_rgb,
                                      const float* g_depth, const float* g_w, float* g_raw, float* g_rays, hipStream_t stream);
int sn_sample_pdf_launch(const float* z_vals, const float* weights, const float* u, long n_rays, int n_samples,
                         int n_importance, float* z_fine, float* z_merged, hipStream_t stream);
int sn_sample_pdf_bins_launch(const float* bins, const float* weights, const float* u, long n_rays, int n_bins,
                              int n_importance, float eps, float* samples, hipStream_t stream);
// the steps around the hot path (sn_next.hip) and the ray gradients (sn_ray_grad.hip)
int sn_generate_rays_launch(const float* c2w, int H, int W, float focal, float near, float far, int x0, int y0, int sx,
                            int sy, int pw, int ph, float* rays, hipStream_t stream);
long sn_generate_rays_backward_workspace_bytes_impl();
int sn_generate_rays_backward_launch(const float* g_rays, int H, int W, float focal, int x0, int y0, int sx, int sy, int pw,
                                     int ph, void* workspace, float* g_c2w, hipStream_t stream);
// ... the same for any of the reference's cameras (fx, fy, cx, cy, sign convention) with the optional NDC stage, and the NDC map on
// its own; a_x = -1/(W/(2 focal)), a_y = -1/(H/(2 focal)) arrive computed in double (sn_api.hip)
// intr / focal != NULL: the intrinsics are read from DEVICE memory (fx, fy, cx, cy; one focal length for the NDC map alone), the
// floats given for them are ignored and a_x, a_y are formed on the device from H, W; the backwards then write g_intr / g_focal too
int sn_generate_rays_cam_launch(const float* c2w, float fx, float fy, float cx, float cy, int convention, int ndc, float ax, float ay,
                                float ndc_near, float near, float far, int x0, int y0, int sx, int sy, int pw, int ph, float* rays,
                                const float* intr, int H, int W, hipStream_t stream);
long sn_camera_backward_workspace_bytes_impl();
int sn_generate_rays_cam_backward_launch(const float* g_rays, const float* c2w, float fx, float fy, float cx, float cy, int convention,
                                         int ndc, float ax, float ay, float ndc_near, int x0, int y0, int sx, int sy, int pw, int ph,
                                         void* workspace, float* g_c2w, const float* intr, int H, int W, float* g_intr,
                                         hipStream_t stream);
int sn_ndc_rays_launch(const float* rays_in, long n_rays, float ax, float ay, float ndc_near, float* rays_out, const float* focal, int H,
                       int W, hipStream_t stream);
int sn_ndc_rays_backward_launch(const float* rays_in, const float* g_rays_out, long n_rays, float ax, float ay, float ndc_near,
                                float* g_rays_in, const float* focal, int H, int W, void* workspace, float* g_focal,
                                hipStream_t stream);
// the optimisers over the flat buffers (sn_optim.hip); the scalars of SGD / RAdam / Ranger arrive in double and are rounded to fp32 once.
int sn_adam_step_launch(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                        float wd, int step, hipStream_t stream);
// sn_radam_step_launch: slow == nullptr is RAdam, otherwise Ranger (lookahead into slow when sync != 0)
int sn_sgd_step_launch(float* p, const float* g, float* buf, long n, double lr, double momentum, double wd, hipStream_t stream);
int sn_radam_step_launch(float* p, const float* g, float* m, float* v, long n, double b1, double b2, double eps, double decay,
                         double step_coeff, int rectified, float* slow, double alpha, int sync, hipStream_t stream);
long sn_render_loss_workspace_bytes_impl();
int sn_render_loss_launch(const float* rgb_c, const float* rgb_f, const float* depth_c, const float* depth_f,
                          const float* rgb_gt, const float* depth_gt, const unsigned char* mask, int mask_mode, long n,
                          float w_rgb, float w_depth, float* g_rgb_c, float* g_rgb_f, float* g_depth_c, float* g_depth_f,
                          void* workspace, float* out, hipStream_t stream);
long sn_ray_grads_workspace_bytes_impl(long n_rays, int n_samples);
int sn_ray_grads_launch(const float* w1, const float* w5, const float* wdir, int layout, const void* g_acts, long slot_rows,
                        const float* rays, const float* z_vals, long n_rays, int n_samples, void* workspace, float* g_rays,
                        hipStream_t stream);
// ... and the per-point position gradients with their weighted sum over a ray's samples (sn_ray_grad.hip)
int sn_point_grads_launch(const float* w1, const float* w5, int layout, const void* g_acts, long slot_rows, const float* rays,
                          const float* z_vals, long n_rays, int n_samples, float* g_xyz, hipStream_t stream);
int sn_point_grads_wsum_launch(const float* g_xyz, const float* weights, long n_rays, int n_samples, float* g_sum,
                               hipStream_t stream);
// the losses on the rendered patches (sn_patch_loss.hip); *_blocks_impl: partial records the first kernel writes
long sn_patch_loss_blocks_impl(int B, int H, int W, int C, int use_ssim);
long sn_patch_loss_workspace_bytes_impl(int B, int H, int W, int C, int use_ssim);
int sn_patch_loss_launch(const float* coarse, const float* fine, const float* target, int B, int H, int W, int C, int use_ssim, int window,
                         float w_mse, float w_ssim, float* g_coarse, float* g_fine, void* workspace, float* out, hipStream_t stream);
long sn_depth_smoothness_workspace_bytes_impl();
int sn_depth_smoothness_launch(const float* idepth, const float* image, int B, int H, int W, int C, float* g_idepth, float* g_image,
                               void* workspace, float* out, hipStream_t stream);
// the regularisers on a ray's compositing weights (sn_ray_reg.hip)
long sn_ray_regularizers_workspace_bytes_impl(long n_rays);
int sn_ray_regularizers_launch(const float* weights, const float* z_vals, const float* rays, long n_rays, int n_samples, float w_dist,
                               float w_ent, float ent_threshold, float* g_weights, float* per_ray, void* workspace, float* out,
                               hipStream_t stream);
// the unseen-view reprojection loss: the inverse warp of a render into the reference camera (sn_reproject.hip)
long sn_reproject_loss_workspace_bytes_impl(long n);
int sn_reproject_loss_launch(const float* rays, const float* depth, const float* rgb, const float* opacity, long n, int C,
                             const float* ref_image, const float* ref_depth, int H, int W, const double* ref_proj, float occ_tol,
                             float charb_eps, float z_min, float opacity_threshold, float w_photo, float w_free, float* g_depth,
                             float* g_rgb, float* per_pixel, unsigned char* flags, void* workspace, float* out, hipStream_t stream);
// the unseen-view forward warp and the draw among the landed pixels (sn_warp.hip)
long sn_forward_warp_workspace_bytes_impl(int H, int W);
int sn_forward_warp_launch(const float* ref_depth, const float* data, int H, int W, int C, const double* ref_proj, const double* src_proj,
                           double eps, int mode, int x0, int y0, int stride_x, int stride_y, int out_w, int out_h, float* out_new,
                           float* new_depth, unsigned char* mask, int* winner, void* workspace, hipStream_t stream);
long sn_select_landed_workspace_bytes_impl(long n);
int sn_select_landed_launch(const unsigned char* mask, long n, const float* u, long m, int* idx, int* n_landed, void* workspace,
                            hipStream_t stream);
// the one-image sampler: window origins with content, strided windows out of full frames (sn_sampler.hip)
long sn_valid_windows_workspace_bytes_impl(int H, int nx);
int sn_valid_windows_launch(const unsigned char* mask, int H, int W, int stride_x, int stride_y, int patch_w, int patch_h, int nx, int ny,
                            unsigned char* valid, int* n_valid, void* workspace, hipStream_t stream);
int sn_gather_windows_launch(const void* const* src, void* const* dst, const int* channels, int n_src, unsigned planar_mask, int H, int W,
                             const int* origin, int stride_x, int stride_y, int patch_w, int patch_h, hipStream_t stream);
}  // extern "C"
