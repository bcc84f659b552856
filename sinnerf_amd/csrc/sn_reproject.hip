// sn_reproject.hip -- the unseen-view reprojection loss (gfx950): the inverse warp of the unseen-view render into the reference camera.
//
// One thread per pixel of the render.  The pixel is lifted along its own (WORLD space) ray by the depth the network rendered,
// X = o + t d, projected with the reference camera's [K E[:3]; 0 0 0 1] matrix, q = P X, (u, v) = (q0, q1) / q2, and the reference image
// and depth are sampled bilinearly there (integer pixel coordinates are sample positions, as in sn_warp.hip):
//
//   photometric term   Charbonnier distance of the rendered colour to the sampled one, over the pixels the reference camera SEES
//                      (|z - D| <= occ_tol D: the view-synthesis loss of SfMLearner / MonoDepth2 with an occlusion test)
//   free-space term    max(0, (D - z) / D - occ_tol): a rendered surface in front of what the reference camera saw is a floater
//
// with the gradient to the rendered colour and -- through the sampling coordinates -- to the rendered depth.  include/sinnerf_hip.h states
// the definitions.  Every mask is a constant for the gradient; rays, the reference frame and the matrix receive none.
//
// The means divide by counts only the whole batch knows, so the work is two launches in the form of sn_patch_loss.hip: reproject_stats_kernel
// (values, per_pixel, flags, per-block partial sums) and reproject_grad_kernel, whose every block re-reduces the at most STAT_BLOCKS partial
// records in index order -- the same bits in every block -- before it scales its pixels' gradients; block 0 writes the scalars.  The
// per-pixel chain is evaluated again in the second launch instead of being kept: ~200 fp64 operations against 8 + 4 C doubles of
// workspace traffic per pixel, and no workspace that grows with n.  All arithmetic is fp64 on the fp32 inputs (u = q0 / z and z - D cancel
// in fp32), ONE rounding to fp32 where a value leaves; sums with the helpers of sn_wave.h, no atomics: the same bits on every call.
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_wave.h"

namespace snj {

constexpr int N_SUMS = 5;                        // per-block partial record: sum photo over V, sum free over G, n_vis, n_geo, n_front
constexpr int STAT_BLOCKS = 256;                 // grid cap of reproject_stats_kernel = the most partial records a block re-reduces
constexpr int GRAD_BLOCKS = 1024;                // grid cap of reproject_grad_kernel
constexpr int MAX_C = 4;

struct Params {
  const float* rays; const float* depth; const float* rgb; const float* opacity;
  const float* ref_image; const float* ref_depth; const double* P;
  long n; int C, H, W;
  double occ_tol, eps2, z_min, opacity_threshold;
};

struct Pixel {
  bool G, V, front;
  double photo, free_;                           // the per-pixel terms, 0 where their mask is off
  double gd_photo, gd_free;                      // d photo_i / d t and d free_i / d t, unscaled
  double s[MAX_C];                               // d (C photo_i) / d rgb_ic
};

// GRADS: also the derivatives (the second launch); the masks and values are the same instructions in both instantiations
template <bool GRADS>
SN_DEV Pixel eval_pixel(const Params& p, long i) {
  Pixel r;
  r.G = r.V = r.front = false;
  r.photo = r.free_ = r.gd_photo = r.gd_free = 0.0;
#pragma unroll
  for (int c = 0; c < MAX_C; ++c) r.s[c] = 0.0;
  const float tf = p.depth[i];
  if (!(isfinite(tf) && tf > 0.0f)) return r;
  if (p.opacity != nullptr && !((double)p.opacity[i] > p.opacity_threshold)) return r;
  const float* ray = p.rays + i * 8;
  const double t = (double)tf;
  const double dx = (double)ray[3], dy = (double)ray[4], dz = (double)ray[5];
  const double X0 = (double)ray[0] + t * dx, X1 = (double)ray[1] + t * dy, X2 = (double)ray[2] + t * dz;
  const double* P = p.P;
  const double q0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
  const double q1 = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
  const double z = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
  if (!(z >= p.z_min)) return r;
  const double u = q0 / z, v = q1 / z;
  const int W = p.W, H = p.H, C = p.C;
  if (!(u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1))) return r;      // false for NaN: no read below leaves the frame
  int x0 = (int)floor(u), y0 = (int)floor(v);
  x0 = x0 > W - 2 ? W - 2 : x0;
  y0 = y0 > H - 2 ? H - 2 : y0;
  const double fx = u - (double)x0, fy = v - (double)y0;
  const long i00 = (long)y0 * W + x0, i10 = i00 + 1, i01 = i00 + W, i11 = i01 + 1;
  const float d00f = p.ref_depth[i00], d10f = p.ref_depth[i10], d01f = p.ref_depth[i01], d11f = p.ref_depth[i11];
  if (!(d00f > 0.0f && d10f > 0.0f && d01f > 0.0f && d11f > 0.0f)) return r;                  // a zero depth is background
  r.G = true;
  const double d00 = (double)d00f, d10 = (double)d10f, d01 = (double)d01f, d11 = (double)d11f;
  const double D = (1.0 - fy) * ((1.0 - fx) * d00 + fx * d10) + fy * ((1.0 - fx) * d01 + fx * d11);
  const double res = (z - D) / D;
  r.V = fabs(res) <= p.occ_tol;
  const double fr = -res - p.occ_tol;
  r.front = fr > 0.0;
  r.free_ = r.front ? fr : 0.0;
  if (!r.V && !(GRADS && r.front)) return r;
  double u_t = 0.0, v_t = 0.0, a2 = 0.0;
  if (GRADS) {
    const double a0 = (P[0] * dx + P[1] * dy) + P[2] * dz, a1 = (P[4] * dx + P[5] * dy) + P[6] * dz;
    a2 = (P[8] * dx + P[9] * dy) + P[10] * dz;
    u_t = (a0 - u * a2) / z;
    v_t = (a1 - v * a2) / z;
    if (r.front) {
      const double D_u = (1.0 - fy) * (d10 - d00) + fy * (d11 - d01), D_v = (1.0 - fx) * (d01 - d00) + fx * (d11 - d10);
      const double r_t = a2 / D - z * (D_u * u_t + D_v * v_t) / (D * D);
      r.gd_free = -r_t;
    }
  }
  if (r.V) {
    double acc = 0.0, gacc = 0.0;
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) {
      if (c >= C) break;
      const double c00 = (double)p.ref_image[i00 * C + c], c10 = (double)p.ref_image[i10 * C + c];
      const double c01 = (double)p.ref_image[i01 * C + c], c11 = (double)p.ref_image[i11 * C + c];
      const double cs = (1.0 - fy) * ((1.0 - fx) * c00 + fx * c10) + fy * ((1.0 - fx) * c01 + fx * c11);
      const double e = (double)p.rgb[i * C + c] - cs, h = sqrt(e * e + p.eps2);
      acc += h;
      if (GRADS) {
        const double c_u = (1.0 - fy) * (c10 - c00) + fy * (c11 - c01), c_v = (1.0 - fx) * (c01 - c00) + fx * (c11 - c10);
        r.s[c] = e / h;
        gacc += r.s[c] * (c_u * u_t + c_v * v_t);
      }
    }
    r.photo = acc / (double)C;
    r.gd_photo = -gacc / (double)C;
  }
  return r;
}

__global__ void __launch_bounds__(256)
reproject_stats_kernel(Params p, float* __restrict__ per_pixel, unsigned char* __restrict__ flags, double* __restrict__ partials) {
  __shared__ double sh[4];
  double acc[N_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (long)gridDim.x * blockDim.x) {
    const Pixel px = eval_pixel<false>(p, i);
    acc[0] += px.photo;
    acc[1] += px.free_;
    acc[2] += px.V ? 1.0 : 0.0;
    acc[3] += px.G ? 1.0 : 0.0;
    acc[4] += px.front ? 1.0 : 0.0;
    if (per_pixel != nullptr) {
      float2 o;
      o.x = (float)px.photo; o.y = (float)px.free_;
      reinterpret_cast<float2*>(per_pixel)[i] = o;
    }
    if (flags != nullptr) flags[i] = (unsigned char)((px.G ? 1 : 0) | (px.V ? 2 : 0) | (px.front ? 4 : 0));
  }
  snwv::write_block_partials(acc, sh, partials);
}

// every block: the partial records summed in index order (snwv::sum_partials), then its pixels' gradients; block 0: out[6]
__global__ void __launch_bounds__(256)
reproject_grad_kernel(Params p, const double* __restrict__ partials, int n_partials, float w_photo, float w_free,
                      float* __restrict__ g_depth, float* __restrict__ g_rgb, float* __restrict__ out) {
  __shared__ double sh[4];
  double tot[N_SUMS];
  snwv::sum_partials(partials, (long)n_partials, sh, tot);
  const double n_vis = tot[2], n_geo = tot[3];
  if (g_depth != nullptr || g_rgb != nullptr) {
    const double k_photo = n_vis > 0.0 ? (double)w_photo / n_vis : 0.0, k_free = n_geo > 0.0 ? (double)w_free / n_geo : 0.0;
    const int C = p.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (long)gridDim.x * blockDim.x) {
      const Pixel px = eval_pixel<true>(p, i);
      if (g_depth != nullptr) {
        const double gp = px.V ? k_photo * px.gd_photo : 0.0, gf = px.front ? k_free * px.gd_free : 0.0;
        g_depth[i] = (float)(gp + gf);
      }
      if (g_rgb != nullptr) {
#pragma unroll
        for (int c = 0; c < MAX_C; ++c) {
          if (c >= C) break;
          g_rgb[i * C + c] = px.V ? (float)(k_photo * px.s[c] / (double)C) : 0.0f;
        }
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double photo = n_vis > 0.0 ? tot[0] / n_vis : 0.0, free_ = n_geo > 0.0 ? tot[1] / n_geo : 0.0;
    out[0] = (float)photo;
    out[1] = (float)free_;
    out[2] = (float)((double)w_photo * photo + (double)w_free * free_);
    out[3] = (float)n_vis;
    out[4] = (float)n_geo;
    out[5] = (float)tot[4];
  }
}

}  // namespace snj

extern "C" long sn_reproject_loss_workspace_bytes_impl(long n) {
  return (long)snh::stride_grid_min1(n, snj::STAT_BLOCKS) * (long)(snj::N_SUMS * sizeof(double));
}

extern "C" int sn_reproject_loss_launch(const float* rays, const float* depth, const float* rgb, const float* opacity, long n, int C,
                                        const float* ref_image, const float* ref_depth, int H, int W, const double* ref_proj,
                                        float occ_tol, float charb_eps, float z_min, float opacity_threshold, float w_photo, float w_free,
                                        float* g_depth, float* g_rgb, float* per_pixel, unsigned char* flags, void* workspace,
                                        float* out, hipStream_t stream) {
  using namespace snj;
  if (n <= 0) return (int)hipMemsetAsync(out, 0, 6 * sizeof(float), stream);
  Params p;
  p.rays = rays; p.depth = depth; p.rgb = rgb; p.opacity = opacity;
  p.ref_image = ref_image; p.ref_depth = ref_depth; p.P = ref_proj;
  p.n = n; p.C = C; p.H = H; p.W = W;
  p.occ_tol = (double)occ_tol;
  p.eps2 = (double)charb_eps * (double)charb_eps;
  p.z_min = (double)z_min;
  p.opacity_threshold = (double)opacity_threshold;
  double* partials = reinterpret_cast<double*>(workspace);
  const unsigned stat_blocks = snh::stride_grid(n, STAT_BLOCKS);
  const unsigned grad_blocks = (g_depth != nullptr || g_rgb != nullptr) ? snh::stride_grid(n, GRAD_BLOCKS) : 1u;
  hipLaunchKernelGGL(reproject_stats_kernel, dim3(stat_blocks), dim3(256), 0, stream, p, per_pixel, flags, partials);
  hipLaunchKernelGGL(reproject_grad_kernel, dim3(grad_blocks), dim3(256), 0, stream, p, partials, (int)stat_blocks, w_photo, w_free,
                     g_depth, g_rgb, out);
  return (int)hipGetLastError();
}
