// sn_ray_reg.hip -- regularisers on the distribution of the compositing weights along a ray (gfx950), one 64-lane wave per ray:
//
//   distortion loss   Mip-NeRF 360, eq. 15   dist = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
//   ray entropy       InfoNeRF, eqs. 5-7     H = -sum_i p_i log(p_i + 1e-10), p = w / (sum w + 1e-10), masked by sum w > threshold
//
// on the normalised depths s = (z - near) / (far - near), with m the interval mid points and d the interval lengths (the last sample
// has m = s and d = 0: the compositor's 1e10 last delta is not a length).  include/sinnerf_hip.h states the definitions.
//
// m is non-decreasing, so the double sum needs no double loop: with W, M the prefix / suffix sums of w and of w m
//     A_k = sum_j w_j |m_k - m_j| = m_k (W_<k - W_>k) - (M_<k - M_>k)       dist = sum_k w_k A_k + ...       d dist / d w_k = 2 A_k + (2/3) w_k d_k
// -- two wave scans.  The layout is the compositor's (sn_render.hip): lane l owns the C consecutive samples [l C, (l + 1) C).  All
// arithmetic is fp64 on the fp32 inputs, in-lane running sums and cross-lane scans in a fixed order, ONE rounding to fp32 where a value
// leaves.  Reductions over the rays with the helpers of sn_wave.h: per-block partials in double, re-reduced in index order by a second
// launch -- no atomics, the same bits on every call.
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_wave.h"

namespace snq {

using snwv::wave_incl_scan_add;
using snwv::wave_sum;

constexpr int N_SUMS = 3;                        // per-block partial record: sum dist, sum ent, rays with the mask set

template <int C>
__global__ void __launch_bounds__(256)
ray_reg_kernel(const float* __restrict__ weights, const float* __restrict__ z_vals, const float* __restrict__ rays, long n_rays, int S,
               float w_dist, float w_ent, float ent_threshold, float* __restrict__ g_weights, float* __restrict__ per_ray,
               double* __restrict__ partials) {
  __shared__ double sh[4][N_SUMS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long ray = (long)blockIdx.x * 4 + wv;
  double r_dist = 0.0, r_ent = 0.0, r_mask = 0.0;
  if (ray < n_rays) {                            // wave-uniform; the waves of a block meet again at the barrier below
    const float near = rays[ray * 8 + 6], far = rays[ray * 8 + 7];
    const double nr = (double)near;
    const double inv = far > near ? 1.0 / ((double)far - nr) : 0.0;
    const long base = ray * (long)S;
    const int i0 = lane * C;

    // s_c for the C owned samples and the one after them (the next lane's first); recomputed, not kept, in the second pass
    float zf[C + 1], wf[C];
#pragma unroll
    for (int c = 0; c < C + 1; ++c) zf[c] = (i0 + c < S) ? z_vals[base + i0 + c] : 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) wf[c] = (i0 + c < S) ? weights[base + i0 + c] : 0.0f;
    double lw = 0.0, lwm = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int i = i0 + c;
      const double s = ((double)zf[c] - nr) * inv, sn = ((double)zf[c + 1] - nr) * inv;
      const double m = (i < S - 1) ? 0.5 * (s + sn) : s;
      const double w = (double)wf[c];                     // 0 for a pad sample (i >= S): it adds nothing anywhere below
      lw += w;
      lwm += w * m;
    }
    const double incl_w = wave_incl_scan_add(lw, lane), incl_m = wave_incl_scan_add(lwm, lane);
    const double tot_w = __shfl(incl_w, 63, 64), tot_m = __shfl(incl_m, 63, 64);
    const double q = tot_w + 1e-10;
    double pre_w = incl_w - lw, pre_m = incl_m - lwm;     // exclusive prefixes of this lane's first sample
    double gd[C], h[C];
    double dist = 0.0, ent = 0.0, hp = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int i = i0 + c;
      const double s = ((double)zf[c] - nr) * inv, sn = ((double)zf[c + 1] - nr) * inv;
      const double m = (i < S - 1) ? 0.5 * (s + sn) : s;
      const double d = (i < S - 1) ? sn - s : 0.0;
      const double w = (double)wf[c], wm = w * m;
      // W_<k - W_>k = 2 W_<k + w_k - W, and the same for M
      const double A = m * (2.0 * pre_w + w - tot_w) - (2.0 * pre_m + wm - tot_m);
      dist += w * A + (1.0 / 3.0) * (w * w) * d;
      gd[c] = 2.0 * A + (2.0 / 3.0) * w * d;
      pre_w += w;
      pre_m += wm;
      const double p = w / q, pe = p + 1e-10, lg = log(pe);
      ent -= p * lg;
      h[c] = -(lg + p / pe);
      hp += h[c] * p;
    }
    dist = wave_sum(dist);
    ent = wave_sum(ent);
    hp = wave_sum(hp);
    const bool mask = tot_w > (double)ent_threshold;
    if (g_weights != nullptr) {
      const double kd = (double)w_dist, ke = mask ? (double)w_ent : 0.0, inv_n = 1.0 / (double)n_rays;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int i = i0 + c;
        if (i < S) g_weights[base + i] = (float)((kd * gd[c] + ke * ((h[c] - hp) / q)) * inv_n);
      }
    }
    r_dist = dist;
    r_ent = mask ? ent : 0.0;
    r_mask = mask ? 1.0 : 0.0;
    if (per_ray != nullptr && lane == 0) {
      float2 o;
      o.x = (float)r_dist; o.y = (float)r_ent;
      reinterpret_cast<float2*>(per_ray)[ray] = o;
    }
  }
  // not snwv::write_block_partials: each wave holds ONE finished value per sum (its ray's), so the four are combined behind a single
  // barrier, left to right as block_sum does it, instead of a butterfly and two barriers per sum
  if (lane == 0) { sh[wv][0] = r_dist; sh[wv][1] = r_ent; sh[wv][2] = r_mask; }
  __syncthreads();
  if (threadIdx.x < N_SUMS) {
    const int k = threadIdx.x;
    partials[(long)blockIdx.x * N_SUMS + k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
  }
}

// one block: the partial records summed in index order (snwv::sum_partials)
__global__ void __launch_bounds__(256)
ray_reg_finish_kernel(const double* __restrict__ partials, long n_partials, long n_rays, float w_dist, float w_ent,
                      float* __restrict__ out) {
  __shared__ double sh[4];
  double t[N_SUMS];
  snwv::sum_partials(partials, n_partials, sh, t);
  if (threadIdx.x == 0) {
    const double n = (double)n_rays, md = t[0] / n, me = t[1] / n;
    out[0] = (float)md;
    out[1] = (float)me;
    out[2] = (float)((double)w_dist * md + (double)w_ent * me);
    out[3] = (float)t[2];
  }
}

}  // namespace snq

extern "C" long sn_ray_regularizers_workspace_bytes_impl(long n_rays) {
  const long blocks = snh::ray_blocks(n_rays);
  return (blocks < 1 ? 1 : blocks) * (long)(snq::N_SUMS * sizeof(double));
}

extern "C" int sn_ray_regularizers_launch(const float* weights, const float* z_vals, const float* rays, long n_rays, int n_samples,
                                          float w_dist, float w_ent, float ent_threshold, float* g_weights, float* per_ray,
                                          void* workspace, float* out, hipStream_t stream) {
  using namespace snq;
  if (n_rays <= 0) return (int)hipMemsetAsync(out, 0, 4 * sizeof(float), stream);
  const int C = snh::samples_per_lane(n_samples);
  if (!C) return SN_E_BADSHAPE;
  dim3 grid, block(256);
  if (const int refused = snh::ray_grid(n_rays, &grid)) return refused;
  double* partials = reinterpret_cast<double*>(workspace);
  snh::for_samples_per_lane(C, [&](auto c) {
    hipLaunchKernelGGL((ray_reg_kernel<decltype(c)::value>), grid, block, 0, stream, weights, z_vals, rays, n_rays, n_samples, w_dist,
                       w_ent, ent_threshold, g_weights, per_ray, partials);
  });
  hipLaunchKernelGGL(ray_reg_finish_kernel, dim3(1), dim3(256), 0, stream, partials, (long)grid.x, n_rays, w_dist, w_ent, out);
  return (int)hipGetLastError();
}
