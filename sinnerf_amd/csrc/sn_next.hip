// sn_next.hip -- the steps immediately before / after the hot path (SURVEY.md §8f "next" rows), gfx950.
//
//   generate_rays_kernel   datasets/ray_utils.py:86-133 (get_ray_directions + get_rays) and the [o, d, near, far] packing
//                          of the datasets (blender_ray_patch_1image_rot3d.py:201-211, strided patches :487-498):
//                          rays are produced ON the GPU from (c2w, focal) -- no (H*W, 8) host array, no H2D copy.
//   rays_bwd_*_kernel      the backward of generate_rays_kernel w.r.t. c2w (pose gradients): 12 deterministic sums over the rays.
//   generate_rays_cam_kernel / rays_cam_bwd_partials_kernel / ndc_rays_kernel / ndc_rays_bwd_kernel
//                          the two above for the reference's other cameras: separate fx, fy, a principal point and the OpenCV
//                          signs of dtu (datasets/dtu_proj.py:17-35), and the NDC map of llff (datasets/ray_utils.py:123-164)
//                          with its adjoint, fused into ray generation / the pose sums or over an existing (n, 8) ray array.
//                          As templates: <true> reads the intrinsics from DEVICE memory (a learnable focal length: no host
//                          read) and the backwards add the sums of dL/d(fx, fy, cx, cy); <false> is the host-float code as before.
//   loss_partials_kernel / loss_finish_kernel
//                          the losses computed on the rendered rays right after the path: MSE coarse + fine
//                          (losses.py:12-22, nn.MSELoss mean), SmoothL1 depth coarse + fine (models/sinnerf.py:32-42 SL1Loss,
//                          call sites :310-319) and PSNR (metrics.py:5-15), together with dLoss/d{rgb,depth}_{coarse,fine}
//                          -- two small launches instead of ~20 elementwise/reduction launches and their HBM round trips.
// All are HBM-bound elementwise kernels: coalesced, 16-byte accesses where the layout allows.
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_wave.h"

namespace snx {

// pixel (x = x0 + ix*sx, y = y0 + iy*sy), ix < pw, iy < ph, row-major over (iy, ix).
__global__ void __launch_bounds__(256)
generate_rays_kernel(const float* __restrict__ c2w, int H, int W, float focal, float near, float far, int x0, int y0,
                     int sx, int sy, int pw, int ph, float* __restrict__ rays) {
  const long total = (long)pw * ph;
  const float r00 = c2w[0], r01 = c2w[1], r02 = c2w[2], tx = c2w[3];
  const float r10 = c2w[4], r11 = c2w[5], r12 = c2w[6], ty = c2w[7];
  const float r20 = c2w[8], r21 = c2w[9], r22 = c2w[10], tz = c2w[11];
  const float hw = (float)W / 2.0f, hh = (float)H / 2.0f;      // Python: W/2, H/2 (true division)
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int iy = (int)(idx / pw), ix = (int)(idx - (long)iy * pw);
    const float i = (float)(x0 + ix * sx), j = (float)(y0 + iy * sy);
    // directions = [(i - W/2)/focal, -(j - H/2)/focal, -1]                                  ray_utils.py:89-91
    const float d0 = __fdiv_rn(__fsub_rn(i, hw), focal);
    const float d1 = -__fdiv_rn(__fsub_rn(j, hh), focal);
    const float d2 = -1.0f;
    // rays_d = directions @ c2w[:, :3].T  (left-to-right accumulation of the 3 products)   ray_utils.py:109
    float4 lo, hi;
    lo.x = tx; lo.y = ty; lo.z = tz;                                                         // rays_o = c2w[:, 3]  :112
    lo.w = __fadd_rn(__fadd_rn(__fmul_rn(d0, r00), __fmul_rn(d1, r01)), __fmul_rn(d2, r02));
    hi.x = __fadd_rn(__fadd_rn(__fmul_rn(d0, r10), __fmul_rn(d1, r11)), __fmul_rn(d2, r12));
    hi.y = __fadd_rn(__fadd_rn(__fmul_rn(d0, r20), __fmul_rn(d1, r21)), __fmul_rn(d2, r22));
    hi.z = near; hi.w = far;
    float4* out = reinterpret_cast<float4*>(rays + idx * 8);
    out[0] = lo; out[1] = hi;
  }
}

// ---- losses on the rendered rays ---------------------------------------------------------------------------------
// Deterministic two-phase reduction (sn_wave.h): every block accumulates its grid-stride share in double and writes 5 partials
// (sum (rgb_c-gt)^2, sum (rgb_f-gt)^2, sum sl1(depth_c-gt), sum sl1(depth_f-gt), number of depth elements counted);
// the finish kernel re-reduces the <= LOSS_BLOCKS partials in index order in every block (so each block knows the
// normalisers) and writes the gradients; block 0 writes the scalars.
constexpr int LOSS_BLOCKS = 256;

SN_DEV bool depth_counted(const float* depth_gt, const unsigned char* mask, int mask_mode, long i) {
  // SL1Loss.forward: mask given -> it; mask None and useMask -> depth_gt > 0; useMask=False -> everything
  return mask_mode == 0 ? true : (mask_mode == 1 ? depth_gt[i] > 0.0f : mask[i] != 0);
}

__global__ void __launch_bounds__(256)
loss_partials_kernel(const float* __restrict__ rgb_c, const float* __restrict__ rgb_f, const float* __restrict__ depth_c,
                     const float* __restrict__ depth_f, const float* __restrict__ rgb_gt,
                     const float* __restrict__ depth_gt, const unsigned char* __restrict__ mask, int mask_mode, long n,
                     double* __restrict__ partials) {
  __shared__ double sh[4];
  double a[5] = {0, 0, 0, 0, 0};
  const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (rgb_gt != nullptr)
    for (long i = t0; i < 3 * n; i += stride) {
      const float g = rgb_gt[i];
      if (rgb_c != nullptr) { const float d = rgb_c[i] - g; a[0] += (double)(d * d); }
      if (rgb_f != nullptr) { const float d = rgb_f[i] - g; a[1] += (double)(d * d); }
    }
  if (depth_gt != nullptr)
    for (long i = t0; i < n; i += stride) {
      if (!depth_counted(depth_gt, mask, mask_mode, i)) continue;
      const float g = depth_gt[i];
      if (depth_c != nullptr) { const float d = fabsf(depth_c[i] - g); a[2] += (double)(d < 1.0f ? 0.5f * d * d : d - 0.5f); }
      if (depth_f != nullptr) { const float d = fabsf(depth_f[i] - g); a[3] += (double)(d < 1.0f ? 0.5f * d * d : d - 0.5f); }
      a[4] += 1.0;
    }
  snwv::write_block_partials(a, sh, partials);
}

// out[8] = mse_coarse, mse_fine, sl1_coarse, sl1_fine, total = w_rgb (mse_c + mse_f) + w_depth (sl1_c + sl1_f),
//          psnr_coarse, psnr_fine, depth elements counted.  Gradients are those of `total`.
__global__ void __launch_bounds__(256)
loss_finish_kernel(const float* __restrict__ rgb_c, const float* __restrict__ rgb_f, const float* __restrict__ depth_c,
                   const float* __restrict__ depth_f, const float* __restrict__ rgb_gt,
                   const float* __restrict__ depth_gt, const unsigned char* __restrict__ mask, int mask_mode, long n,
                   float w_rgb, float w_depth, const double* __restrict__ partials, int n_partials,
                   float* __restrict__ g_rgb_c, float* __restrict__ g_rgb_f, float* __restrict__ g_depth_c,
                   float* __restrict__ g_depth_f, float* __restrict__ out) {
  __shared__ double sh[4];
  double tot[5];
  snwv::sum_partials(partials, n_partials, sh, tot);
  const double n_rgb = 3.0 * (double)n, n_d = tot[4];
  const float mse_c = rgb_c && rgb_gt ? (float)(tot[0] / n_rgb) : 0.0f, mse_f = rgb_f && rgb_gt ? (float)(tot[1] / n_rgb) : 0.0f;
  const float sl_c = depth_c && depth_gt ? (float)(tot[2] / n_d) : 0.0f, sl_f = depth_f && depth_gt ? (float)(tot[3] / n_d) : 0.0f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = mse_c; out[1] = mse_f; out[2] = sl_c; out[3] = sl_f;
    out[4] = w_rgb * (mse_c + mse_f) + w_depth * (sl_c + sl_f);
    out[5] = -10.0f * log10f(mse_c); out[6] = -10.0f * log10f(mse_f);            // metrics.py:14-15
    out[7] = (float)n_d;
  }
  const float s_rgb = (float)((double)w_rgb * 2.0 / n_rgb), s_d = (float)((double)w_depth / n_d);
  const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (rgb_gt != nullptr)
    for (long i = t0; i < 3 * n; i += stride) {
      const float g = rgb_gt[i];
      if (g_rgb_c != nullptr && rgb_c != nullptr) g_rgb_c[i] = s_rgb * (rgb_c[i] - g);
      if (g_rgb_f != nullptr && rgb_f != nullptr) g_rgb_f[i] = s_rgb * (rgb_f[i] - g);
    }
  if (depth_gt != nullptr)
    for (long i = t0; i < n; i += stride) {
      const bool on = depth_counted(depth_gt, mask, mask_mode, i);
      const float g = depth_gt[i];
      if (g_depth_c != nullptr && depth_c != nullptr) {
        const float d = depth_c[i] - g;
        g_depth_c[i] = on ? s_d * (fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f)) : 0.0f;
      }
      if (g_depth_f != nullptr && depth_f != nullptr) {
        const float d = depth_f[i] - g;
        g_depth_f[i] = on ? s_d * (fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f)) : 0.0f;
      }
    }
}

// ---- backward of generate_rays_kernel w.r.t. c2w (autograd of ray_utils.py:109, :112: rays_d = directions @ c2w[:, :3].T,
// rays_o = c2w[:, 3] expanded):  g_c2w[a][b] = sum_rays g_d[a] * dir_cam[b],  g_c2w[a][3] = sum_rays g_o[a].
// Two phases like the loss reduction above: per-block fp64 partials of the 12 sums over a grid-stride share, then one block
// adds the <= RAYS_BWD_BLOCKS partials in index order -- deterministic, no atomics.
constexpr int RAYS_BWD_BLOCKS = 256;

__global__ void __launch_bounds__(256)
rays_bwd_partials_kernel(const float* __restrict__ g_rays, int H, int W, float focal, int x0, int y0, int sx, int sy, int pw,
                         int ph, double* __restrict__ partials) {
  __shared__ double sh[4];
  const long total = (long)pw * ph;
  const float hw = (float)W / 2.0f, hh = (float)H / 2.0f;
  double a[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int iy = (int)(idx / pw), ix = (int)(idx - (long)iy * pw);
    const float i = (float)(x0 + ix * sx), j = (float)(y0 + iy * sy);
    const double d0 = (double)__fdiv_rn(__fsub_rn(i, hw), focal), d1 = (double)(-__fdiv_rn(__fsub_rn(j, hh), focal)), d2 = -1.0;
    const float4* g = reinterpret_cast<const float4*>(g_rays + idx * 8);
    const float4 lo = g[0], hi = g[1];
    const double go[3] = {(double)lo.x, (double)lo.y, (double)lo.z}, gd[3] = {(double)lo.w, (double)hi.x, (double)hi.y};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      a[4 * r + 0] += gd[r] * d0; a[4 * r + 1] += gd[r] * d1; a[4 * r + 2] += gd[r] * d2; a[4 * r + 3] += go[r];
    }
  }
  snwv::write_block_partials(a, sh, partials);
}

__global__ void __launch_bounds__(256)
rays_bwd_finish_kernel(const double* __restrict__ partials, int n_partials, float* __restrict__ g_c2w) {
  __shared__ double sh[4];
  double tot[12];
  snwv::sum_partials(partials, n_partials, sh, tot);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 12; ++k) g_c2w[k] = (float)tot[k];
}

// ---- the reference's other cameras: llff (get_ndc_rays, datasets/ray_utils.py:123-164) and dtu (get_ray_directions_dtu,
// datasets/dtu_proj.py:17-35) -------------------------------------------------------------------------------------------
struct Camera {
  float fx, fy, cx, cy;
  int convention;                  // 0: ((i-cx)/fx, -(j-cy)/fy, -1)  ray_utils.py:89-91;  1: ((i-cx)/fx, (j-cy)/fy, +1)  dtu_proj.py:31-33
  int ndc;                         // 1: the rays go through the NDC map below
  float ax, ay, ndc_near, two_near;// -1/(W/(2 focal)), -1/(H/(2 focal)), near, 2 near: the reference's Python floats, cast once
};
struct Window { int x0, y0, sx, sy, pw, ph; };

// The intrinsics held in DEVICE memory (a learnable focal length: no host read, no sync).  a_x, a_y as ndc_scale forms them on the
// host (sn_api.hip): in fp64 with one cast; __ddiv_rn so that no flag can change them.  2.0 * focal is exact.
SN_DEV float ndc_scale_dev(int size, float focal) { return (float)__ddiv_rn(-1.0, __ddiv_rn((double)size, 2.0 * (double)focal)); }
SN_DEV void camera_ndc_focal(Camera& cam, float focal, int H, int W) { cam.ax = ndc_scale_dev(W, focal); cam.ay = ndc_scale_dev(H, focal); }
// intr = (fx, fy, cx, cy); the NDC map's focal length is fx
SN_DEV void camera_intrinsics(Camera& cam, const float* intr, int H, int W) {
  cam.fx = intr[0]; cam.fy = intr[1]; cam.cx = intr[2]; cam.cy = intr[3];
  camera_ndc_focal(cam, intr[0], H, W);
}

SN_DEV void camera_dir(const Camera& cam, const Window& win, long idx, float& d0, float& d1, float& d2) {
  const int iy = (int)(idx / win.pw), ix = (int)(idx - (long)iy * win.pw);
  const float i = (float)(win.x0 + ix * win.sx), j = (float)(win.y0 + iy * win.sy);
  d0 = __fdiv_rn(__fsub_rn(i, cam.cx), cam.fx);
  const float v = __fdiv_rn(__fsub_rn(j, cam.cy), cam.fy);
  d1 = cam.convention ? v : -v;
  d2 = cam.convention ? 1.0f : -1.0f;
}

// rays_d = directions @ c2w[:, :3].T, left to right as generate_rays_kernel does                       ray_utils.py:109
SN_DEV void rotate(const float* R, float d0, float d1, float d2, float* d) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    d[a] = __fadd_rn(__fadd_rn(__fmul_rn(d0, R[4 * a + 0]), __fmul_rn(d1, R[4 * a + 1])), __fmul_rn(d2, R[4 * a + 2]));
}

// the quotients of get_ndc_rays that a_x, a_y scale, one rounding per torch op
struct NdcRatios { float pz, ox_oz, oy_oz, u, v; };
SN_DEV NdcRatios ndc_ratios(const Camera& cam, const float* o, const float* d) {
  NdcRatios q;
  const float t = __fdiv_rn(-__fadd_rn(cam.ndc_near, o[2]), d[2]);                                        // :145
  const float px = __fadd_rn(o[0], __fmul_rn(t, d[0])), py = __fadd_rn(o[1], __fmul_rn(t, d[1]));         // :146
  q.pz = __fadd_rn(o[2], __fmul_rn(t, d[2]));
  q.ox_oz = __fdiv_rn(px, q.pz); q.oy_oz = __fdiv_rn(py, q.pz);                                           // :149-150
  q.u = __fdiv_rn(d[0], d[2]); q.v = __fdiv_rn(d[1], d[2]);
  return q;
}

// get_ndc_rays op by op, one rounding per torch op (scalar / tensor is tensor.reciprocal() * scalar in torch)
SN_DEV void ndc_map(const Camera& cam, float* o, float* d) {
  const NdcRatios q = ndc_ratios(cam, o, d);
  const float o2 = __fadd_rn(1.0f, __fmul_rn(__fdiv_rn(1.0f, q.pz), cam.two_near));                       // :155
  o[0] = __fmul_rn(cam.ax, q.ox_oz); o[1] = __fmul_rn(cam.ay, q.oy_oz); o[2] = o2;                        // :153-154
  d[0] = __fmul_rn(cam.ax, __fsub_rn(q.u, q.ox_oz)); d[1] = __fmul_rn(cam.ay, __fsub_rn(q.v, q.oy_oz));   // :157-158
  d[2] = __fsub_rn(1.0f, o2);                                                                             // :159
}

// The adjoint of ndc_map as autograd derives it from :145-159, fp32, forward intermediates recomputed.  pz is only approximately
// -near: its derivative terms stay.  o, d: the map's INPUT; go, gd: in = gradient of the map's output, out = gradient of its input.
SN_DEV void ndc_map_adjoint(const Camera& cam, const float* o, const float* d, float* go, float* gd) {
  const float t = __fdiv_rn(-__fadd_rn(cam.ndc_near, o[2]), d[2]);
  const float px = __fadd_rn(o[0], __fmul_rn(t, d[0])), py = __fadd_rn(o[1], __fmul_rn(t, d[1])),
              pz = __fadd_rn(o[2], __fmul_rn(t, d[2]));
  const float rz = __fdiv_rn(1.0f, pz), ox_oz = __fdiv_rn(px, pz), oy_oz = __fdiv_rn(py, pz);
  const float u = __fdiv_rn(d[0], d[2]), v = __fdiv_rn(d[1], d[2]);
  // d2 = 1 - o2, o2 = 1 + rz * two_near
  const float g_rz = (go[2] - gd[2]) * cam.two_near;
  // o0 = ax ox_oz, d0 = ax (u - ox_oz); o1, d1 alike
  const float g_u = cam.ax * gd[0], g_v = cam.ay * gd[1];
  const float g_a = cam.ax * go[0] - g_u, g_b = cam.ay * go[1] - g_v;
  // ox_oz = px / pz, oy_oz = py / pz, rz = 1 / pz
  const float g_px = g_a / pz, g_py = g_b / pz;
  const float g_pz = (-g_rz * (rz * rz) - g_a * ox_oz / pz) - g_b * oy_oz / pz;
  // u = dx / dz, v = dy / dz
  float g_dx = g_u / d[2], g_dy = g_v / d[2], g_dz = -g_u * u / d[2] - g_v * v / d[2];
  // p = o + t d
  const float g_t = (g_px * d[0] + g_py * d[1]) + g_pz * d[2];
  g_dx += t * g_px; g_dy += t * g_py; g_dz += t * g_pz;
  // t = -(near + oz) / dz
  g_dz -= g_t * t / d[2];
  go[0] = g_px; go[1] = g_py; go[2] = g_pz - g_t / d[2];
  gd[0] = g_dx; gd[1] = g_dy; gd[2] = g_dz;
}

// generate_rays_kernel for any of the cameras; (convention 0, fx = fy = focal, cx = W/2, cy = H/2, ndc 0) writes its bits.
// DEV: the four intrinsics and a_x, a_y come from intr (DEVICE) instead of cam; everything after that is the same code.
template <bool DEV>
__global__ void __launch_bounds__(256)
generate_rays_cam_kernel(const float* __restrict__ c2w, Camera cam, const float* __restrict__ intr, int H, int W, float near, float far,
                         Window win, float* __restrict__ rays) {
  const long total = (long)win.pw * win.ph;
  if (DEV) camera_intrinsics(cam, intr, H, W);
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = c2w[k];
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    float d0, d1, d2, o[3] = {R[3], R[7], R[11]}, d[3];                                    // rays_o = c2w[:, 3]  ray_utils.py:114
    camera_dir(cam, win, idx, d0, d1, d2);
    rotate(R, d0, d1, d2, d);
    if (cam.ndc) ndc_map(cam, o, d);
    float4* out = reinterpret_cast<float4*>(rays + idx * 8);
    out[0] = make_float4(o[0], o[1], o[2], d[0]); out[1] = make_float4(d[1], d[2], near, far);
  }
}

// the NDC map over rays that exist already (n, 8); columns 6, 7 pass through.  One thread reads its whole ray before it writes
// it: rays_out may be rays_in (no __restrict__)
template <bool DEV>
__global__ void __launch_bounds__(256)
ndc_rays_kernel(const float* rays_in, long n, Camera cam, const float* __restrict__ focal, int H, int W, float* rays_out) {
  if (DEV) camera_ndc_focal(cam, focal[0], H, W);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const float4* in = reinterpret_cast<const float4*>(rays_in + idx * 8);
    const float4 lo = in[0], hi = in[1];
    float o[3] = {lo.x, lo.y, lo.z}, d[3] = {lo.w, hi.x, hi.y};
    ndc_map(cam, o, d);
    float4* out = reinterpret_cast<float4*>(rays_out + idx * 8);
    out[0] = make_float4(o[0], o[1], o[2], d[0]); out[1] = make_float4(d[1], d[2], hi.z, hi.w);
  }
}

// The sums behind dL/d(fx, fy, cx, cy), next to the 12 pose sums; a_x = -2 focal / W and a_y = -2 focal / H are summed on their own
// and folded into the focal length by the finish kernel.
constexpr int CAM_SUMS = 18;       // 12 pose sums, g_fx, g_fy, g_cx, g_cy, g_ax, g_ay
constexpr int NDC_SUMS = 2;        // g_ax, g_ay: the NDC map on its own

// d(a_x ox_oz, a_y oy_oz, ., a_x (u - ox_oz), a_y (v - oy_oz), .) / d(a_x, a_y) against the gradient (go, gd) of the map's OUTPUT,
// from the fp32 quantities the forward computes; products and sums in fp64
SN_DEV void ndc_scale_sums(const Camera& cam, const float* o, const float* d, const float* go, const float* gd, double& g_ax, double& g_ay) {
  const NdcRatios q = ndc_ratios(cam, o, d);
  g_ax += (double)go[0] * (double)q.ox_oz + (double)gd[0] * (double)__fsub_rn(q.u, q.ox_oz);
  g_ay += (double)go[1] * (double)q.oy_oz + (double)gd[1] * (double)__fsub_rn(q.v, q.oy_oz);
}

// FOCAL: the focal length comes from DEVICE memory and its gradient is wanted: per-block partials of g_ax, g_ay (NDC_SUMS) as well
template <bool FOCAL>
__global__ void __launch_bounds__(256)
ndc_rays_bwd_kernel(const float* __restrict__ rays_in, const float* __restrict__ g_out, long n, Camera cam,
                    const float* __restrict__ focal, int H, int W, float* __restrict__ g_in, double* __restrict__ partials) {
  __shared__ double sh[4];
  if (FOCAL) camera_ndc_focal(cam, focal[0], H, W);
  double g_a[NDC_SUMS] = {0.0, 0.0};             // g_ax, g_ay
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const float4* in = reinterpret_cast<const float4*>(rays_in + idx * 8);
    const float4* g = reinterpret_cast<const float4*>(g_out + idx * 8);
    const float4 lo = in[0], hi = in[1], glo = g[0], ghi = g[1];
    const float o[3] = {lo.x, lo.y, lo.z}, d[3] = {lo.w, hi.x, hi.y};
    float go[3] = {glo.x, glo.y, glo.z}, gd[3] = {glo.w, ghi.x, ghi.y};
    if (FOCAL) ndc_scale_sums(cam, o, d, go, gd, g_a[0], g_a[1]);
    ndc_map_adjoint(cam, o, d, go, gd);
    float4* out = reinterpret_cast<float4*>(g_in + idx * 8);
    out[0] = make_float4(go[0], go[1], go[2], gd[0]); out[1] = make_float4(gd[1], gd[2], 0.0f, 0.0f);
  }
  if (FOCAL) snwv::write_block_partials(g_a, sh, partials);
}

// rays_bwd_partials_kernel for any of the cameras: with ndc on, the upstream gradient of each ray first goes back through the
// NDC map (the world ray is recomputed from c2w as generate_rays_cam_kernel computes it), in registers.  The sums, their order
// and the finish kernel are those of rays_bwd_partials_kernel.
// INTR: the intrinsics come from intr (DEVICE) and their sums follow the 12 (CAM_SUMS per block): with c the camera direction,
// gc = R^T gd the gradient of it and s the sign of the convention,  c0 = (i - cx) / fx,  c1 = s (j - cy) / fy  give
//   g_fx += gc0 (-c0 / fx)   g_cx += gc0 (-1 / fx)   g_fy += gc1 (-c1 / fy)   g_cy += gc1 (-s / fy)
// c2w is then always read.  The first 12 sums are the same expressions over the same rays in the same order either way.
template <bool INTR>
__global__ void __launch_bounds__(256)
rays_cam_bwd_partials_kernel(const float* __restrict__ g_rays, const float* __restrict__ c2w, Camera cam,
                             const float* __restrict__ intr, int H, int W, Window win, double* __restrict__ partials) {
  constexpr int NS = INTR ? CAM_SUMS : 12;
  __shared__ double sh[4];
  const long total = (long)win.pw * win.ph;
  if (INTR) camera_intrinsics(cam, intr, H, W);
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = (INTR || cam.ndc) ? c2w[k] : 0.0f;
  double a[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = 0.0;
  const double fx = (double)cam.fx, fy = (double)cam.fy, s = cam.convention ? 1.0 : -1.0;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    float c0, c1, c2;
    camera_dir(cam, win, idx, c0, c1, c2);
    const double d0 = (double)c0, d1 = (double)c1, d2 = (double)c2;
    const float4* g = reinterpret_cast<const float4*>(g_rays + idx * 8);
    const float4 lo = g[0], hi = g[1];
    float gof[3] = {lo.x, lo.y, lo.z}, gdf[3] = {lo.w, hi.x, hi.y};
    if (cam.ndc) {
      const float o[3] = {R[3], R[7], R[11]};
      float d[3];
      rotate(R, c0, c1, c2, d);
      if constexpr (INTR) ndc_scale_sums(cam, o, d, gof, gdf, a[NS - 2], a[NS - 1]);
      ndc_map_adjoint(cam, o, d, gof, gdf);
    }
    const double go[3] = {(double)gof[0], (double)gof[1], (double)gof[2]}, gd[3] = {(double)gdf[0], (double)gdf[1], (double)gdf[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      a[4 * r + 0] += gd[r] * d0; a[4 * r + 1] += gd[r] * d1; a[4 * r + 2] += gd[r] * d2; a[4 * r + 3] += go[r];
    }
    if constexpr (INTR) {
      const double gc0 = (gd[0] * (double)R[0] + gd[1] * (double)R[4]) + gd[2] * (double)R[8];
      const double gc1 = (gd[0] * (double)R[1] + gd[1] * (double)R[5]) + gd[2] * (double)R[9];
      a[12] += gc0 * (-d0 / fx); a[13] += gc1 * (-d1 / fy); a[14] += gc0 * (-1.0 / fx); a[15] += gc1 * (-s / fy);
    }
  }
  snwv::write_block_partials(a, sh, partials);
}

// rays_bwd_finish_kernel for NS sums per block: the <= RAYS_BWD_BLOCKS partials added in index order, then
//   CAM_SUMS: g_c2w (12) and g_intr = (g_fx + g_ax sx + g_ay sy, g_fy, g_cx, g_cy);   NDC_SUMS: g_intr[0] = g_ax sx + g_ay sy,
// sx = da_x / dfocal = -2 / W, sy = -2 / H.  An output that is NULL is not written.
template <int NS>
__global__ void __launch_bounds__(256)
rays_intr_bwd_finish_kernel(const double* __restrict__ partials, int n_partials, double sx, double sy, float* __restrict__ g_c2w,
                            float* __restrict__ g_intr) {
  __shared__ double sh[4];
  double tot[NS];
  snwv::sum_partials(partials, n_partials, sh, tot);
  if (threadIdx.x != 0) return;
  if constexpr (NS == CAM_SUMS) {
    if (g_c2w != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) g_c2w[k] = (float)tot[k];
    }
    if (g_intr != nullptr) {
      g_intr[0] = (float)((tot[12] + tot[NS - 2] * sx) + tot[NS - 1] * sy);
      g_intr[1] = (float)tot[13]; g_intr[2] = (float)tot[14]; g_intr[3] = (float)tot[15];
    }
  } else {
    g_intr[0] = (float)(tot[NS - 2] * sx + tot[NS - 1] * sy);
  }
}

}  // namespace snx

extern "C" int sn_generate_rays_launch(const float* c2w, int H, int W, float focal, float near, float far, int x0, int y0,
                                       int sx, int sy, int pw, int ph, float* rays, hipStream_t stream) {
  const long total = (long)pw * ph;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(snx::generate_rays_kernel, dim3(snh::stride_grid(total, 4096)), dim3(256), 0, stream, c2w, H, W, focal, near, far,
                     x0, y0, sx, sy, pw, ph, rays);
  return (int)hipGetLastError();
}

extern "C" long sn_generate_rays_backward_workspace_bytes_impl() { return (long)snx::RAYS_BWD_BLOCKS * 12 * sizeof(double); }
extern "C" int sn_generate_rays_backward_launch(const float* g_rays, int H, int W, float focal, int x0, int y0, int sx, int sy,
                                                int pw, int ph, void* workspace, float* g_c2w, hipStream_t stream) {
  using namespace snx;
  const long total = (long)pw * ph;
  const unsigned blocks = snh::stride_grid_min1(total, RAYS_BWD_BLOCKS);       // an empty window still writes its 12 zeros
  double* partials = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(rays_bwd_partials_kernel, dim3(blocks), dim3(256), 0, stream, g_rays, H, W, focal, x0, y0, sx, sy,
                     pw, ph, partials);
  hipLaunchKernelGGL(rays_bwd_finish_kernel, dim3(1), dim3(256), 0, stream, partials, (int)blocks, g_c2w);
  return (int)hipGetLastError();
}

static snx::Camera make_camera(float fx, float fy, float cx, float cy, int convention, int ndc, float ax, float ay, float ndc_near) {
  return snx::Camera{fx, fy, cx, cy, convention, ndc, ax, ay, ndc_near, (float)(2.0 * (double)ndc_near)};
}

// intr != NULL in the four launches below: the intrinsics (one focal length for the NDC map on its own) are read from DEVICE memory by
// the kernel and the floats given for them are ignored; H, W then form a_x, a_y on the device.
extern "C" int sn_generate_rays_cam_launch(const float* c2w, float fx, float fy, float cx, float cy, int convention, int ndc, float ax,
                                           float ay, float ndc_near, float near, float far, int x0, int y0, int sx, int sy, int pw,
                                           int ph, float* rays, const float* intr, int H, int W, hipStream_t stream) {
  using namespace snx;
  const long total = (long)pw * ph;
  if (total <= 0) return 0;
  const unsigned blocks = snh::stride_grid(total, 4096);
  const Camera cam = make_camera(fx, fy, cx, cy, convention, ndc, ax, ay, ndc_near);
  const Window win{x0, y0, sx, sy, pw, ph};
  if (intr != nullptr)
    hipLaunchKernelGGL(generate_rays_cam_kernel<true>, dim3(blocks), dim3(256), 0, stream, c2w, cam, intr, H, W, near, far, win, rays);
  else
    hipLaunchKernelGGL(generate_rays_cam_kernel<false>, dim3(blocks), dim3(256), 0, stream, c2w, cam, intr, H, W, near, far, win, rays);
  return (int)hipGetLastError();
}

extern "C" long sn_camera_backward_workspace_bytes_impl() { return (long)snx::RAYS_BWD_BLOCKS * snx::CAM_SUMS * sizeof(double); }
// intr == NULL: g_intr is not used, the workspace is that of sn_generate_rays_backward and c2w is read only with ndc
extern "C" int sn_generate_rays_cam_backward_launch(const float* g_rays, const float* c2w, float fx, float fy, float cx, float cy,
                                                    int convention, int ndc, float ax, float ay, float ndc_near, int x0, int y0, int sx,
                                                    int sy, int pw, int ph, void* workspace, float* g_c2w, const float* intr, int H, int W,
                                                    float* g_intr, hipStream_t stream) {
  using namespace snx;
  const long total = (long)pw * ph;
  const unsigned blocks = snh::stride_grid_min1(total, RAYS_BWD_BLOCKS);       // an empty window still writes its zeros
  double* partials = reinterpret_cast<double*>(workspace);
  const Camera cam = make_camera(fx, fy, cx, cy, convention, ndc, ax, ay, ndc_near);
  const Window win{x0, y0, sx, sy, pw, ph};
  if (intr != nullptr) {
    hipLaunchKernelGGL(rays_cam_bwd_partials_kernel<true>, dim3(blocks), dim3(256), 0, stream, g_rays, c2w, cam, intr, H, W, win,
                       partials);
    hipLaunchKernelGGL(rays_intr_bwd_finish_kernel<CAM_SUMS>, dim3(1), dim3(256), 0, stream, partials, (int)blocks, -2.0 / (double)W,
                       -2.0 / (double)H, g_c2w, g_intr);
  } else {
    hipLaunchKernelGGL(rays_cam_bwd_partials_kernel<false>, dim3(blocks), dim3(256), 0, stream, g_rays, c2w, cam, intr, H, W, win,
                       partials);
    hipLaunchKernelGGL(rays_bwd_finish_kernel, dim3(1), dim3(256), 0, stream, partials, (int)blocks, g_c2w);
  }
  return (int)hipGetLastError();
}

extern "C" int sn_ndc_rays_launch(const float* rays_in, long n_rays, float ax, float ay, float ndc_near, float* rays_out,
                                  const float* focal, int H, int W, hipStream_t stream) {
  using namespace snx;
  if (n_rays <= 0) return 0;
  const unsigned blocks = snh::stride_grid(n_rays, 4096);
  const Camera cam = make_camera(1.0f, 1.0f, 0.0f, 0.0f, 0, 1, ax, ay, ndc_near);
  if (focal != nullptr)
    hipLaunchKernelGGL(ndc_rays_kernel<true>, dim3(blocks), dim3(256), 0, stream, rays_in, n_rays, cam, focal, H, W, rays_out);
  else
    hipLaunchKernelGGL(ndc_rays_kernel<false>, dim3(blocks), dim3(256), 0, stream, rays_in, n_rays, cam, focal, H, W, rays_out);
  return (int)hipGetLastError();
}

// focal != NULL: g_focal (1 float) is written as well, through workspace (sn_camera_backward_workspace_bytes); no rays: g_focal = 0
extern "C" int sn_ndc_rays_backward_launch(const float* rays_in, const float* g_rays_out, long n_rays, float ax, float ay,
                                           float ndc_near, float* g_rays_in, const float* focal, int H, int W, void* workspace,
                                           float* g_focal, hipStream_t stream) {
  using namespace snx;
  const Camera cam = make_camera(1.0f, 1.0f, 0.0f, 0.0f, 0, 1, ax, ay, ndc_near);
  if (focal != nullptr) {
    const unsigned blocks = snh::stride_grid_min1(n_rays, RAYS_BWD_BLOCKS);
    double* partials = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(ndc_rays_bwd_kernel<true>, dim3(blocks), dim3(256), 0, stream, rays_in, g_rays_out, n_rays, cam, focal, H,
                       W, g_rays_in, partials);
    hipLaunchKernelGGL(rays_intr_bwd_finish_kernel<NDC_SUMS>, dim3(1), dim3(256), 0, stream, partials, (int)blocks, -2.0 / (double)W,
                       -2.0 / (double)H, (float*)nullptr, g_focal);
    return (int)hipGetLastError();
  }
  if (n_rays <= 0) return 0;
  hipLaunchKernelGGL(ndc_rays_bwd_kernel<false>, dim3(snh::stride_grid(n_rays, 4096)), dim3(256), 0, stream, rays_in, g_rays_out, n_rays, cam, focal, H, W,
                     g_rays_in, (double*)nullptr);
  return (int)hipGetLastError();
}

extern "C" long sn_render_loss_workspace_bytes_impl() { return (long)snx::LOSS_BLOCKS * 5 * sizeof(double); }
extern "C" int sn_render_loss_launch(const float* rgb_c, const float* rgb_f, const float* depth_c, const float* depth_f,
                                     const float* rgb_gt, const float* depth_gt, const unsigned char* mask, int mask_mode,
                                     long n, float w_rgb, float w_depth, float* g_rgb_c, float* g_rgb_f, float* g_depth_c,
                                     float* g_depth_f, void* workspace, float* out, hipStream_t stream) {
  using namespace snx;
  const unsigned blocks = snh::stride_grid_min1(3 * n, LOSS_BLOCKS);
  double* partials = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(loss_partials_kernel, dim3(blocks), dim3(256), 0, stream, rgb_c, rgb_f, depth_c, depth_f,
                     rgb_gt, depth_gt, mask, mask_mode, n, partials);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(blocks), dim3(256), 0, stream, rgb_c, rgb_f, depth_c, depth_f,
                     rgb_gt, depth_gt, mask, mask_mode, n, w_rgb, w_depth, partials, (int)blocks, g_rgb_c, g_rgb_f,
                     g_depth_c, g_depth_f, out);
  return (int)hipGetLastError();
}
