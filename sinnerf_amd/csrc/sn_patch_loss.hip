// sn_patch_loss.hip -- the losses the reference computes on the rendered PATCHES right after the hot path, gfx950:
//
//   ssim_stats_kernel / patch_grad_kernel<true>     losses.py:94-109 L2_SSIM_Loss: nn.MSELoss 'mean' of coarse and fine against the
//                                                   target + w_ssim x kornia 0.6.3 ssim_loss(fine, target, window) (gaussian window,
//                                                   sigma 1.5, reflect padding, eps 1e-12, mean of clamp((1 - ssim) / 2, 0, 1))
//   mse_partials_kernel / patch_grad_kernel<false>  the MSE pair alone on any channel count (losses.py:12-22 on 4-D patches)
//   smooth_kernel / smooth_finish_kernel            kornia inverse_depth_smoothness_loss(idepth, image), gradients to both
//
// Everything is read and written CHANNEL-LAST, (B, H, W, C): the (B*H*W, C) rows render_rays returns and its (B*H*W,) depth vectors, so
// no permute copy stands between the renderer and the loss.  Patches are 64 x 64 or 56 x 70: the cost is launches, not arithmetic, and
// the arithmetic is spent on accuracy instead -- window sums, the SSIM quotient, its partial derivatives and the adjoint filter are fp64
// (F(a a) - mu^2 cancels, and at a == b the three adjoint terms cancel each other); one rounding to fp32 where a value leaves.
// Reductions with the helpers of sn_wave.h: per-block partials in double, re-reduced in index order -- deterministic, no atomics.
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_wave.h"

namespace snp {

constexpr int TILE = 16;                         // a block of ssim_stats_kernel owns TILE x TILE pixels of one image
constexpr int MAX_R = SN_PATCH_LOSS_MAX_WINDOW / 2;
constexpr int REG = TILE + 2 * MAX_R;            // the tile with its halo
constexpr int FLAT_BLOCKS = 256;                 // grid cap of the grid-stride kernels (= partial records they write)

struct Taps { double g[2 * MAX_R + 1]; };        // the normalised 1-D gaussian, formed on the host in double

// index of torch's reflect padding for e in [-r, n - 1 + r], r < n; clamped so that no caller can leave the plane
SN_DEV int reflect(int e, int n) {
  const int i = e < 0 ? -e : (e >= n ? 2 * (n - 1) - e : e);
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// ---- forward: one block per (image, tile), channels in turn.  The tile's halo is loaded with the reflected indices resolved, the five
// planes a, b, a a, a b, b b are filtered along x into LDS and along y into registers.  Per pixel: the loss element and the partial
// derivatives of g_scale * ssim with respect to mu1, F(a a) and F(a b) -- with sigma11 = F(a a) - mu1^2 and sigma12 = F(a b) - mu1 mu2
// substituted, so the three are all patch_grad_kernel needs.  partials[3 block + k] = sum (coarse - t)^2, sum (fine - t)^2, sum of the
// loss elements over the tile.
__global__ void __launch_bounds__(256)
ssim_stats_kernel(const float* __restrict__ coarse, const float* __restrict__ fine, const float* __restrict__ target, int H, int W,
                  int C, int r, Taps taps, int tiles_x, int tiles_y, double g_scale, long n_total, double* __restrict__ pqr,
                  double* __restrict__ partials) {
  __shared__ float sa[REG * REG], sb[REG * REG];
  __shared__ double srow[5][REG * TILE];
  __shared__ double sg[2 * MAX_R + 1];
  __shared__ double sh[4];
  const int tid = threadIdx.x, ws = 2 * r + 1, reg = TILE + 2 * r;
  const int per_image = tiles_x * tiles_y;
  const int b = (int)(blockIdx.x / per_image), t = (int)(blockIdx.x - (unsigned)b * per_image);
  const int ty0 = (t / tiles_x) * TILE, tx0 = (t % tiles_x) * TILE;
  const long img = (long)b * H * W;
  if (tid < ws) sg[tid] = taps.g[tid];
  const int ly = tid >> 4, lx = tid & 15, y = ty0 + ly, x = tx0 + lx;
  const bool inside = y < H && x < W;
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, EPS = 1e-12;
  double acc_c = 0.0, acc_f = 0.0, acc_s = 0.0;
  for (int c = 0; c < C; ++c) {
    __syncthreads();                                        // the previous channel's column pass has read srow, sa, sb
    for (int i = tid; i < reg * reg; i += 256) {
      const int ry = i / reg, rx = i - ry * reg, ey = ty0 - r + ry, ex = tx0 - r + rx;
      float va = 0.0f, vb = 0.0f;
      if (ey < H + r && ex < W + r) {                       // beyond: the halo of pixels outside the image, never used
        const long idx = (img + (long)reflect(ey, H) * W + reflect(ex, W)) * C + c;
        va = fine[idx]; vb = target[idx];
      }
      sa[i] = va; sb[i] = vb;
    }
    __syncthreads();
    for (int i = tid; i < reg * TILE; i += 256) {           // along x: region row i / TILE, output column i % TILE
      const int ry = i >> 4, ox = i & 15;
      double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
      for (int k = 0; k < ws; ++k) {
        const double w = sg[k], a = (double)sa[ry * reg + ox + k], bb = (double)sb[ry * reg + ox + k];
        m1 += w * a; m2 += w * bb; e11 += w * (a * a); e22 += w * (bb * bb); e12 += w * (a * bb);
      }
      srow[0][i] = m1; srow[1][i] = m2; srow[2][i] = e11; srow[3][i] = e22; srow[4][i] = e12;
    }
    __syncthreads();
    if (inside) {
      double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
      for (int k = 0; k < ws; ++k) {                        // along y
        const double w = sg[k];
        const int i = (ly + k) * TILE + lx;
        m1 += w * srow[0][i]; m2 += w * srow[1][i]; e11 += w * srow[2][i]; e22 += w * srow[3][i]; e12 += w * srow[4][i];
      }
      const double s11 = e11 - m1 * m1, s22 = e22 - m2 * m2, s12 = e12 - m1 * m2;
      const double A1 = 2.0 * m1 * m2 + C1, A2 = 2.0 * s12 + C2, B1 = m1 * m1 + m2 * m2 + C1, B2 = s11 + s22 + C2;
      const double D = B1 * B2 + EPS, S = A1 * A2 / D;
      const double l = 0.5 * (1.0 - S);
      acc_s += l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);
      const long idx = (img + (long)y * W + x) * C + c;
      const float f = sa[(ly + r) * reg + lx + r], tg = sb[(ly + r) * reg + lx + r];
      const float df = f - tg;
      acc_f += (double)(df * df);
      if (coarse != nullptr) { const float dc = coarse[idx] - tg; acc_c += (double)(dc * dc); }
      if (pqr != nullptr) {
        const double g = (l > 0.0 && l < 1.0) ? g_scale : 0.0;       // the clamp passes gradient strictly inside (0, 1)
        pqr[idx] = g * (2.0 * m2 * (A2 - A1) / D - S * 2.0 * m1 * (B2 - B1) / D);     // d ssim / d mu1
        pqr[n_total + idx] = g * (-S * B1 / D);                                       // d ssim / d F(a a)
        pqr[2 * n_total + idx] = g * (2.0 * A1 / D);                                  // d ssim / d F(a b)
      }
    }
  }
  const double sums[3] = {acc_c, acc_f, acc_s};
  snwv::write_block_partials(sums, sh, partials);
}

// the MSE pair alone: the patch as a flat array of n elements
__global__ void __launch_bounds__(256)
mse_partials_kernel(const float* __restrict__ coarse, const float* __restrict__ fine, const float* __restrict__ target, long n,
                    double* __restrict__ partials) {
  __shared__ double sh[4];
  double acc_c = 0.0, acc_f = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float tg = target[i];
    if (coarse != nullptr) { const float d = coarse[i] - tg; acc_c += (double)(d * d); }
    if (fine != nullptr) { const float d = fine[i] - tg; acc_f += (double)(d * d); }
  }
  const double sums[3] = {acc_c, acc_f, 0.0};
  snwv::write_block_partials(sums, sh, partials);
}

// the pre-images of pixel v under the reflect padding: the extended coordinates e in [-r, n - 1 + r] with reflect(e) == v
SN_DEV int preimages(int v, int n, int r, int* e) {
  int k = 0;
  e[k++] = v;
  if (v >= 1 && v <= r) e[k++] = -v;
  if (v >= n - 1 - r && v <= n - 2) e[k++] = 2 * (n - 1) - v;
  return k;
}

// ---- gradients and scalars.  g_coarse = s_mse (coarse - t); g_fine = s_mse (fine - t) + F^T(p) + 2 a F^T(q) + b F^T(r), where F^T is
// the adjoint of the reflect-padded filter written as a gather: the zero-extended plane filtered at every pre-image of the pixel (the
// halo folded back onto the pixels it reflects from), so every gradient element has one writer.  Block 0 re-reduces the partials of the
// first kernel in index order and writes out[4] = mse_coarse, mse_fine, ssim_loss, w_mse (mse_coarse + mse_fine) + w_ssim ssim_loss.
template <bool SSIM>
__global__ void __launch_bounds__(256)
patch_grad_kernel(const float* __restrict__ coarse, const float* __restrict__ fine, const float* __restrict__ target, int H, int W, int C,
                  int r, Taps taps, long n_total, float w_mse, float w_ssim, const double* __restrict__ pqr,
                  const double* __restrict__ partials, int n_partials, float* __restrict__ g_coarse, float* __restrict__ g_fine,
                  float* __restrict__ out) {
  __shared__ double sg[2 * MAX_R + 1];
  __shared__ double sh[4];
  if (SSIM) {
    if ((int)threadIdx.x < 2 * r + 1) sg[threadIdx.x] = taps.g[threadIdx.x];
    __syncthreads();
  }
  const float s_mse = (float)((double)w_mse * 2.0 / (double)n_total);
  const bool want_c = g_coarse != nullptr && coarse != nullptr, want_f = g_fine != nullptr && fine != nullptr;
  if (want_c || want_f)
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n_total; idx += (long)gridDim.x * blockDim.x) {
      const float tg = target[idx];
      if (want_c) g_coarse[idx] = s_mse * (coarse[idx] - tg);
      if (!want_f) continue;
      const float f = fine[idx];
      const float g_l2 = s_mse * (f - tg);
      if (!SSIM) { g_fine[idx] = g_l2; continue; }
      const long pix = idx / C;
      const int c = (int)(idx - pix * C), x = (int)(pix % W), y = (int)((pix / W) % H);
      const long img = pix - ((long)y * W + x);              // first pixel of this image
      int eys[3], exs[3];
      const int n_ey = preimages(y, H, r, eys), n_ex = preimages(x, W, r, exs);
      double P = 0.0, Q = 0.0, R = 0.0;
      for (int iy = 0; iy < n_ey; ++iy) {
        const int ey = eys[iy], y_lo = ey - r < 0 ? 0 : ey - r, y_hi = ey + r > H - 1 ? H - 1 : ey + r;
        for (int ix = 0; ix < n_ex; ++ix) {
          const int ex = exs[ix], x_lo = ex - r < 0 ? 0 : ex - r, x_hi = ex + r > W - 1 ? W - 1 : ex + r;
          for (int sy = y_lo; sy <= y_hi; ++sy) {
            const double wy = sg[ey - sy + r];
            double p = 0.0, q = 0.0, rr = 0.0;
            for (int sx = x_lo; sx <= x_hi; ++sx) {
              const double wx = sg[ex - sx + r];
              const long s = (img + (long)sy * W + sx) * C + c;
              p += wx * pqr[s]; q += wx * pqr[n_total + s]; rr += wx * pqr[2 * n_total + s];
            }
            P += wy * p; Q += wy * q; R += wy * rr;
          }
        }
      }
      g_fine[idx] = (float)((double)g_l2 + (P + 2.0 * (double)f * Q + (double)tg * R));
    }
  if (blockIdx.x != 0) return;
  double tot[3];
  snwv::sum_partials(partials, n_partials, sh, tot);
  if (threadIdx.x == 0) {
    const double n = (double)n_total;
    const float mse_c = coarse != nullptr ? (float)(tot[0] / n) : 0.0f, mse_f = fine != nullptr ? (float)(tot[1] / n) : 0.0f;
    const float ssim = SSIM ? (float)(tot[2] / n) : 0.0f;
    out[0] = mse_c; out[1] = mse_f; out[2] = ssim;
    out[3] = SSIM ? w_mse * (mse_c + mse_f) + w_ssim * ssim : w_mse * (mse_c + mse_f);
  }
}

// ---- inverse_depth_smoothness_loss.  One thread per pixel: it adds the terms of its right and its lower edge to the sums, and gathers
// the gradient of its own depth and image elements from its (up to) four edges.  edge (A, B): e = d[A] - d[B],
// w = exp(-mean_c |I[A, c] - I[B, c]|), term |e w| = |e| w; d term / d d[A] = sign(e) w, d term / d I[A, c] = -|e| w sign(I[A, c] - I[B, c]) / C
// (sign(0) = 0), both negated for B.
SN_DEV double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

SN_DEV void edge(const float* __restrict__ d, const float* __restrict__ I, long A, long B, int C, double& e, double& w) {
  e = (double)d[A] - (double)d[B];
  double m = 0.0;
  for (int c = 0; c < C; ++c) m += fabs((double)I[A * C + c] - (double)I[B * C + c]);
  w = exp(-m / (double)C);
}

__global__ void __launch_bounds__(256)
smooth_kernel(const float* __restrict__ d, const float* __restrict__ I, long n_pix, int H, int W, int C, double inv_nx, double inv_ny,
              float* __restrict__ g_d, float* __restrict__ g_I, double* __restrict__ partials) {
  __shared__ double sh[4];
  double acc[2] = {0.0, 0.0};                      // the x edges, the y edges
  for (long pix = (long)blockIdx.x * blockDim.x + threadIdx.x; pix < n_pix; pix += (long)gridDim.x * blockDim.x) {
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    // the four edges of this pixel: right, left, down, up.  `first`: this pixel is A of the edge
    const bool valid[4] = {x < W - 1, x > 0, y < H - 1, y > 0};
    const long other[4] = {pix + 1, pix - 1, pix + W, pix - W};
    double gd = 0.0, coef[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      coef[k] = 0.0;
      if (!valid[k]) continue;
      const bool first = (k & 1) == 0;
      double e, w;
      edge(d, I, first ? pix : other[k], first ? other[k] : pix, C, e, w);
      const double inv = k < 2 ? inv_nx : inv_ny;
      if (k == 0) acc[0] += fabs(e) * w;
      if (k == 2) acc[1] += fabs(e) * w;
      gd += (first ? 1.0 : -1.0) * sgn(e) * w * inv;
      coef[k] = -fabs(e) * w * inv / (double)C;              // x sign(I[this, c] - I[other, c]): the same for A and for B
    }
    if (g_d != nullptr) g_d[pix] = (float)gd;
    if (g_I != nullptr)
      for (int c = 0; c < C; ++c) {
        const double v = (double)I[pix * C + c];
        double g = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (valid[k]) g += coef[k] * sgn(v - (double)I[other[k] * C + c]);
        g_I[pix * C + c] = (float)g;
      }
  }
  snwv::write_block_partials(acc, sh, partials);
}

__global__ void __launch_bounds__(256)
smooth_finish_kernel(const double* __restrict__ partials, int n_partials, double inv_nx, double inv_ny, float* __restrict__ out) {
  __shared__ double sh[4];
  double tot[2];
  snwv::sum_partials(partials, n_partials, sh, tot);
  if (threadIdx.x == 0) out[0] = (float)(tot[0] * inv_nx + tot[1] * inv_ny);
}

static Taps make_taps(int window) {                          // gaussian(window, sigma 1.5), normalised to sum 1
  Taps t;
  double sum = 0.0;
  for (int k = 0; k < 2 * MAX_R + 1; ++k) t.g[k] = 0.0;
  for (int k = 0; k < window; ++k) {
    const double x = (double)(k - window / 2);
    t.g[k] = exp(-(x * x) / (2.0 * 1.5 * 1.5));
    sum += t.g[k];
  }
  for (int k = 0; k < window; ++k) t.g[k] /= sum;
  return t;
}

static long flat_blocks(long n) { return (long)snh::stride_grid_min1(n, FLAT_BLOCKS); }
static long tiles_of(int n) { return ((long)n + TILE - 1) / TILE; }

}  // namespace snp

// blocks of the first kernel = partial records
extern "C" long sn_patch_loss_blocks_impl(int B, int H, int W, int C, int use_ssim) {
  return use_ssim ? (long)B * snp::tiles_of(H) * snp::tiles_of(W) : snp::flat_blocks((long)B * H * W * C);
}

extern "C" long sn_patch_loss_workspace_bytes_impl(int B, int H, int W, int C, int use_ssim) {
  const long n = (long)B * H * W * C;
  return (sn_patch_loss_blocks_impl(B, H, W, C, use_ssim) * 3 + (use_ssim ? 3 * n : 0)) * (long)sizeof(double);
}

extern "C" int sn_patch_loss_launch(const float* coarse, const float* fine, const float* target, int B, int H, int W, int C, int use_ssim,
                                    int window, float w_mse, float w_ssim, float* g_coarse, float* g_fine, void* workspace, float* out,
                                    hipStream_t stream) {
  using namespace snp;
  const long n = (long)B * H * W * C, blocks = sn_patch_loss_blocks_impl(B, H, W, C, use_ssim);
  double* partials = reinterpret_cast<double*>(workspace);
  const bool grads = (g_coarse != nullptr && coarse != nullptr) || (g_fine != nullptr && fine != nullptr);
  const unsigned grad_blocks = grads ? snh::stride_grid(n, 4096) : 1u;
  if (use_ssim) {
    const int r = window / 2;
    const Taps taps = make_taps(window);
    double* pqr = g_fine != nullptr ? partials + blocks * 3 : nullptr;
    hipLaunchKernelGGL(ssim_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, coarse, fine, target, H, W, C, r, taps,
                       (int)tiles_of(W), (int)tiles_of(H), -0.5 * (double)w_ssim / (double)n, n, pqr, partials);
    hipLaunchKernelGGL(patch_grad_kernel<true>, dim3(grad_blocks), dim3(256), 0, stream, coarse, fine, target, H, W, C, r, taps, n, w_mse,
                       w_ssim, pqr, partials, (int)blocks, g_coarse, g_fine, out);
  } else {
    hipLaunchKernelGGL(mse_partials_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, coarse, fine, target, n, partials);
    hipLaunchKernelGGL(patch_grad_kernel<false>, dim3(grad_blocks), dim3(256), 0, stream, coarse, fine, target, H, W, C, 0, Taps{}, n,
                       w_mse, w_ssim, nullptr, partials, (int)blocks, g_coarse, g_fine, out);
  }
  return (int)hipGetLastError();
}

extern "C" long sn_depth_smoothness_workspace_bytes_impl() { return (long)snp::FLAT_BLOCKS * 2 * sizeof(double); }

extern "C" int sn_depth_smoothness_launch(const float* idepth, const float* image, int B, int H, int W, int C, float* g_idepth,
                                          float* g_image, void* workspace, float* out, hipStream_t stream) {
  using namespace snp;
  const long n_pix = (long)B * H * W, blocks = flat_blocks(n_pix);
  const double inv_nx = 1.0 / ((double)B * H * (W - 1)), inv_ny = 1.0 / ((double)B * (H - 1) * W);
  double* partials = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, idepth, image, n_pix, H, W, C, inv_nx, inv_ny, g_idepth,
                     g_image, partials);
  hipLaunchKernelGGL(smooth_finish_kernel, dim3(1), dim3(256), 0, stream, partials, (int)blocks, inv_nx, inv_ny, out);
  return (int)hipGetLastError();
}
