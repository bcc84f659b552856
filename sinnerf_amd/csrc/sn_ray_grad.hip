// sn_ray_grad.hip -- gradient of one render pass with respect to the RAYS (origins / directions), gfx950.
//
// The reference's render_rays is differentiable in everything it is given; autograd carries dL/d(raw) back through
// NeRF.forward (models/nerf.py:122-148) to the embedded inputs, through Embedding (nerf.py:36-41) to xyz = o + d z and d
// (models/rendering.py:284-285, :187-190), and sums over the samples of a ray.  Here sn_mlp_backward_chain has already left
// the pre-activation gradients of every layer in g_acts; the three layers that read the embedded input are
//   slot 0  xyz_encoding_1   (256 x 63)            g_emb_xyz  = G0 . W1 + G4 . W5[:, 0:63]     (skip: cat([input_xyz, h]), nerf.py:133)
//   slot 4  xyz_encoding_5   (256 x 319)
//   slot 9  dir_encoding     (128 x 283)           g_emb_dir  = G9[:, 0:128] . Wdir[:, 256:283] (cat([final, input_dir]), nerf.py:142)
// so the ray gradient is one contraction over stored state, P x 512 . 512 x 63 plus P x 128 . 128 x 27, followed by the
// embedding derivative and a sum over samples.  The (P, 90) embedded gradient never reaches HBM.
//
//   ray_grad_points_kernel   v_mfma_f32_32x32x2_f32, features x points: one wave owns 32 points and three 32x32 accumulators
//                            (xyz features 0..31, 32..63, dir features 0..31), a lane ends up with 16 features of ONE point per
//                            accumulator.  The feature order inside a tile is chosen so that a lane holds the sin AND the cos
//                            slot of every (band, axis) it owns: lane half h owns xyz bands 5h..5h+4 and dir bands 2h, 2h+1
//                            (the slot order of embed_xyz / embed_dir in sn_mlp_common.h).  The k order of the dot products is
//                            the order in which a lane's 16-byte loads walk a g_acts row; the weights are staged once per
//                            workgroup in LDS (144 KB) in exactly that order, so an A operand is one ds_read_b128.
//                            Writes a per-point (P, 8) scratch: [g_xyz(3), 0, z g_xyz + g_dirvec (3), 0].
//   ray_grad_reduce_kernel   one wave per ray: fp64 sums over the samples in a fixed order (no atomics) -> g_rays (n_rays, 8).
//
// Arithmetic is fp32 whatever the layout of g_acts (fp32 rows, bf16 rows, or the (hi, lo) pairs of the bf16x3 state).
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_wave.h"

namespace snrg {

constexpr int WAVES = 8;                    // 512 threads: two waves per SIMD share one copy of the weights
constexpr int PTS_WG = WAVES * 32;
constexpr int LDS_FLOATS = 512 * 64 + 128 * 32;

enum { ROW_F32 = 0, ROW_BF16 = 1, ROW_X3 = 2 };     // how a 256-feature row of g_acts is stored

// reference Embedding column (nerf.py:36-41: [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...], groups of 3) of slot e of lane half h
__host__ __device__ constexpr int xyz_col(int h, int e) {
  return e < 30 ? 3 + 6 * (5 * h + (e >> 1) / 3) + 3 * (e & 1) + (e >> 1) % 3 : e == 30 ? (h ? 2 : 0) : (h ? -1 : 1);
}
__host__ __device__ constexpr int dir_col(int h, int e) {
  return e < 12 ? 3 + 6 * (2 * h + (e >> 1) / 3) + 3 * (e & 1) + (e >> 1) % 3 : e == 12 ? (h ? 2 : 0) : e == 13 ? (h ? -1 : 1) : -1;
}

template <int ROW> struct RowTraits;
template <> struct RowTraits<ROW_F32>  { static constexpr int NQ = 4, ROW_BYTES = 1024; };
template <> struct RowTraits<ROW_BF16> { static constexpr int NQ = 8, ROW_BYTES = 512; };
template <> struct RowTraits<ROW_X3>   { static constexpr int NQ = 8, ROW_BYTES = 1024; };

// one 16-byte step of a lane along a row: chunk c holds features [NQ c, NQ c + NQ)
template <int ROW> struct Chunk { uint4 a, b; };
template <int ROW> SN_DEV Chunk<ROW> load_chunk(const char* row, int c) {
  Chunk<ROW> r;
  if (ROW == ROW_X3) {                      // 16 B of hi parts, then 16 B of lo parts (include/sinnerf_hip.h)
    r.a = *reinterpret_cast<const uint4*>(row + 32 * c);
    r.b = *reinterpret_cast<const uint4*>(row + 32 * c + 16);
  } else {
    r.a = *reinterpret_cast<const uint4*>(row + 16 * c);
    r.b = r.a;
  }
  return r;
}
SN_DEV float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
SN_DEV float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
template <int ROW> SN_DEV void decode_chunk(const Chunk<ROW>& r, float* v) {
  const unsigned a[4] = {r.a.x, r.a.y, r.a.z, r.a.w};
  if (ROW == ROW_F32) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = __uint_as_float(a[q]);
  } else if (ROW == ROW_BF16) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[2 * q] = bf_lo(a[q]); v[2 * q + 1] = bf_hi(a[q]); }
  } else {
    const unsigned b[4] = {r.b.x, r.b.y, r.b.z, r.b.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {           // the value a stored pair stands for: hi + lo
      v[2 * q] = __fadd_rn(bf_lo(a[q]), bf_lo(b[q]));
      v[2 * q + 1] = __fadd_rn(bf_hi(a[q]), bf_hi(b[q]));
    }
  }
}

// LDS position of the weight that multiplies feature k (0..255 of one source row) into tile row i:
// [chunk pair t][lane half h][tile][row i][q], the order in which lane (i, h) consumes it
template <int NQ> SN_DEV int lds_pos(int k, int tile, int n_tiles, int i) {
  const int c = k / NQ, q = k % NQ;             // chunk c = 2 t + h
  return ((c * n_tiles + tile) * 32 + i) * NQ + q;
}

// D row i of a 32x32 tile sits in lane half (i >> 2) & 1, register (i & 3) + 4 (i >> 3)
SN_DEV int row_half(int i) { return (i >> 2) & 1; }
SN_DEV int row_reg(int i) { return (i & 3) + 4 * (i >> 3); }

// acc[0..NT) += W^T (NT x 32 features, K deep) . G^T (K x 32 points), K features of one g_acts row per point
template <int ROW, int NT, int K>
SN_DEV void contract(const char* row, const float* lds_w, int lane, f32x16* acc) {
  constexpr int NQ = RowTraits<ROW>::NQ;
  constexpr int U = 32 / NQ;                 // chunks per batch: 32 features per lane half, 64 k per batch
  constexpr int NB = K / 64;
  const int h = lane >> 5, i = lane & 31;
  Chunk<ROW> nxt[U], cur[U];
#pragma unroll
  for (int u = 0; u < U; ++u) nxt[u] = load_chunk<ROW>(row, 2 * u + h);
#pragma unroll 1
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    if (b + 1 < NB) {
#pragma unroll
      for (int u = 0; u < U; ++u) nxt[u] = load_chunk<ROW>(row, 2 * ((b + 1) * U + u) + h);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float v[NQ];
      decode_chunk<ROW>(cur[u], v);
      const int t = b * U + u;
#pragma unroll
      for (int tile = 0; tile < NT; ++tile) {
        const float* ap = lds_w + (((t * 2 + h) * NT + tile) * 32 + i) * NQ;
        float a[NQ];
#pragma unroll
        for (int q4 = 0; q4 < NQ / 4; ++q4) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(ap + 4 * q4);
          a[4 * q4] = w[0]; a[4 * q4 + 1] = w[1]; a[4 * q4 + 2] = w[2]; a[4 * q4 + 3] = w[3];
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[tile] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], v[q], acc[tile], 0, 0, 0);
      }
    }
  }
}

template <int ROWX, int ROWD>
__global__ void __launch_bounds__(WAVES * 64)
ray_grad_points_kernel(const float* __restrict__ w1, const float* __restrict__ w5, const float* __restrict__ wdir,
                       const char* __restrict__ g_acts, long slot_rows, const float* __restrict__ rays,
                       const float* __restrict__ z_vals, long n_points, int S, float* __restrict__ scratch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds_x = reinterpret_cast<float*>(smem);         // xyz weights: source 0 = W1 (k 0..255), source 1 = W5[:, 0:63]
  float* lds_d = lds_x + 512 * 64;                       // dir weights: Wdir[:, 256:283]
  constexpr int NQX = RowTraits<ROWX>::NQ, NQD = RowTraits<ROWD>::NQ;
  constexpr long RBX = RowTraits<ROWX>::ROW_BYTES, RBD = RowTraits<ROWD>::ROW_BYTES;

  // ---- stage the weights once per workgroup (global reads walk the parameter rows; the LDS image is in consumption order)
  for (int idx = threadIdx.x; idx < 512 * 64; idx += WAVES * 64) {
    const int k = idx >> 6, f = idx & 63, tile = f >> 5, i = f & 31;
    const int col = xyz_col(row_half(i), 16 * tile + row_reg(i));
    float w = 0.0f;
    if (col >= 0) w = k < 256 ? w1[k * 63 + col] : w5[(k - 256) * 319 + col];
    lds_x[(k >> 8) * (256 * 64) + lds_pos<NQX>(k & 255, tile, 2, i)] = w;
  }
  for (int idx = threadIdx.x; idx < 128 * 32; idx += WAVES * 64) {
    const int k = idx >> 5, i = idx & 31;
    const int col = dir_col(row_half(i), row_reg(i));
    lds_d[lds_pos<NQD>(k, 0, 1, i)] = col >= 0 ? wdir[k * 283 + 256 + col] : 0.0f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5;
  const long n_tiles = (n_points + PTS_WG - 1) / PTS_WG;
  for (long tile_i = blockIdx.x; tile_i < n_tiles; tile_i += gridDim.x) {
    const long p = tile_i * PTS_WG + wave * 32 + (lane & 31);
    const long pl = p < n_points ? p : n_points - 1;     // rows >= n_points are never read; such a lane's result is dropped
    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    contract<ROWX, 2, 256>(g_acts + (0 * slot_rows + pl) * RBX, lds_x, lane, acc);
    contract<ROWX, 2, 256>(g_acts + (4 * slot_rows + pl) * RBX, lds_x + 256 * 64, lane, acc);
    contract<ROWD, 1, 128>(g_acts + (9 * slot_rows + pl) * RBD, lds_d, lane, acc + 2);

    // ---- embedding derivative (nerf.py:36-41): d/dx sin(2^k x) = 2^k cos(2^k x), d/dx cos(2^k x) = -2^k sin(2^k x)
    const long ray = pl / S;
    const float* rp = rays + ray * 8;
    const float zz = z_vals[pl];
    const float dvx = rp[3], dvy = rp[4], dvz = rp[5];
    // xyz = o + d*z with separate roundings, the point the forward embedded (rendering.py:284-285)
    const float x = __fadd_rn(rp[0], __fmul_rn(dvx, zz)), y = __fadd_rn(rp[1], __fmul_rn(dvy, zz)),
                z = __fadd_rn(rp[2], __fmul_rn(dvz, zz));
    float gx[3] = {0.0f, 0.0f, 0.0f}, gd[3] = {0.0f, 0.0f, 0.0f};
    {
      const Rev2 px = to_revolutions(x), py = to_revolutions(y), pz = to_revolutions(z);
      const float hs = h ? 32.0f : 1.0f;              // bands 5..9 on the upper lane half
#pragma unroll
      for (int pp = 0; pp < 15; ++pp) {
        const Rev2 pc = (pp % 3 == 0) ? px : (pp % 3 == 1) ? py : pz;
        const float scale = hs * (float)(1 << (pp / 3));
        float s, c;
        sincos_rev(pc, scale, s, c);
        const float g_sin = acc[(2 * pp) >> 4][(2 * pp) & 15], g_cos = acc[(2 * pp + 1) >> 4][(2 * pp + 1) & 15];
        gx[pp % 3] += scale * (c * g_sin - s * g_cos);
      }
      if (h) gx[2] += acc[1][14];                      // identity columns: x, y on the lower half, z on the upper
      else { gx[0] += acc[1][14]; gx[1] += acc[1][15]; }
    }
    {
      const Rev2 px = to_revolutions(dvx), py = to_revolutions(dvy), pz = to_revolutions(dvz);
      const float hs = h ? 4.0f : 1.0f;               // bands 2, 3 on the upper lane half
#pragma unroll
      for (int pp = 0; pp < 6; ++pp) {
        const Rev2 pc = (pp % 3 == 0) ? px : (pp % 3 == 1) ? py : pz;
        const float scale = hs * (float)(1 << (pp / 3));
        float s, c;
        sincos_rev(pc, scale, s, c);
        gd[pp % 3] += scale * (c * acc[2][2 * pp] - s * acc[2][2 * pp + 1]);
      }
      if (h) gd[2] += acc[2][12];
      else { gd[0] += acc[2][12]; gd[1] += acc[2][13]; }
    }
    // the two lane halves hold disjoint bands of the same point
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      gx[a] += __shfl_xor(gx[a], 32, 64);
      gd[a] += __shfl_xor(gd[a], 32, 64);
    }
    if (h == 0 && p < n_points) {
      f32x4 lo, hi;
      lo[0] = gx[0]; lo[1] = gx[1]; lo[2] = gx[2]; lo[3] = 0.0f;
      hi[0] = zz * gx[0] + gd[0]; hi[1] = zz * gx[1] + gd[1]; hi[2] = zz * gx[2] + gd[2]; hi[3] = 0.0f;
      f32x4* out = reinterpret_cast<f32x4*>(scratch + p * 8);
      out[0] = lo; out[1] = hi;
    }
  }
}

using snwv::wave_sum;

// g_o = sum_s g_xyz, g_d = sum_s (z g_xyz + g_dirvec): lane l adds samples l, l + 64, ... in order, then the butterfly
__global__ void __launch_bounds__(256)
ray_grad_reduce_kernel(const float* __restrict__ scratch, long n_rays, int S, float* __restrict__ g_rays) {
  const int lane = threadIdx.x & 63;
  const long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;
  double a[6] = {0, 0, 0, 0, 0, 0};
  const f32x4* src = reinterpret_cast<const f32x4*>(scratch + ray * (long)S * 8);
  for (int s = lane; s < S; s += 64) {
    const f32x4 lo = src[2 * s], hi = src[2 * s + 1];
    a[0] += (double)lo[0]; a[1] += (double)lo[1]; a[2] += (double)lo[2];
    a[3] += (double)hi[0]; a[4] += (double)hi[1]; a[5] += (double)hi[2];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = wave_sum(a[k]);
  if (lane == 0) {
    f32x4 lo, hi;
    lo[0] = (float)a[0]; lo[1] = (float)a[1]; lo[2] = (float)a[2]; lo[3] = (float)a[3];
    hi[0] = (float)a[4]; hi[1] = (float)a[5]; hi[2] = 0.0f; hi[3] = 0.0f;          // near / far are constants
    f32x4* out = reinterpret_cast<f32x4*>(g_rays + ray * 8);
    out[0] = lo; out[1] = hi;
  }
}

}  // namespace snrg

extern "C" long sn_ray_grads_workspace_bytes_impl(long n_rays, int n_samples) {
  return n_rays * (long)n_samples * 8 * (long)sizeof(float);
}

// layout: 0 = fp32 rows, 1 = bf16 rows, 2 = bf16x3 state (slots 0..8 (hi, lo) pairs, slot 9 fp32)
extern "C" int sn_ray_grads_launch(const float* w1, const float* w5, const float* wdir, int layout, const void* g_acts,
                                   long slot_rows, const float* rays, const float* z_vals, long n_rays, int n_samples,
                                   void* workspace, float* g_rays, hipStream_t stream) {
  using namespace snrg;
  if (n_rays <= 0) return 0;
  const long n_points = n_rays * (long)n_samples;
  const long tiles = (n_points + PTS_WG - 1) / PTS_WG;
  const unsigned grid = snh::persistent_grid(tiles);
  dim3 rays_grid;
  if (const int refused = snh::ray_grid(n_rays, &rays_grid)) return refused;
  constexpr size_t lds = LDS_FLOATS * sizeof(float);
  float* scratch = reinterpret_cast<float*>(workspace);
  const char* G = reinterpret_cast<const char*>(g_acts);
#define SN_RG(RX, RD)                                                                                            \
  {                                                                                                              \
    SN_ENSURE_DYN_LDS((ray_grad_points_kernel<RX, RD>), lds);                                                    \
    hipLaunchKernelGGL((ray_grad_points_kernel<RX, RD>), dim3(grid), dim3(WAVES * 64), lds, stream, w1, w5, wdir, G, \
                       slot_rows, rays, z_vals, n_points, n_samples, scratch);                                   \
  }
  if (layout == 0) SN_RG(ROW_F32, ROW_F32)
  else if (layout == 1) SN_RG(ROW_BF16, ROW_BF16)
  else SN_RG(ROW_X3, ROW_F32)
#undef SN_RG
  int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(ray_grad_reduce_kernel, rays_grid, dim3(256), 0, stream, scratch, n_rays, n_samples, g_rays);
  return (int)hipGetLastError();
}

// ---- gradients with respect to a POSITION: sn_point_grads / sn_point_grads_wsum --------------------------------------------------------
// The per-point value ray_grad_points_kernel holds before the sum over a ray's samples takes it away, kept: d(out)/d(xyz) of every
// sample point for the upstream gradient the chain was run with (g_raw = (0, 0, 0, 1): the gradient of the raw sigma, nerf.py:136).
//
//   point_grad_kernel        ray_grad_points_kernel without its direction part: the 512 x 64 xyz weights staged once per workgroup
//                            (128 KB of LDS, the same image), `contract` on slots 0 and 4 into two 32x32 accumulators, the Embedding
//                            derivative with the forward's range reduction (sincos_rev_comp below), the half-wave shuffle, ONE 16-byte store per point:
//                            g_xyz (P, 4) = [gx, gy, gz, 0].  Lanes of points >= P read the last real row and store nothing.
//   point_grad_wsum_kernel   one wave per ray: sum_s w[r, s] g_xyz[r, s] in fp64 (the products are exact there), lane-strided, then the
//                            butterfly of ray_grad_reduce_kernel; one rounding to fp32 -> g_sum (n_rays, 4) = [sum, 0].
namespace snrg {

constexpr int LDS_FLOATS_XYZ = 512 * 64;

// sincos_rev (sn_device.h) with the rounding error of its one inexact step carried along.  The forward's range reduction is exact up
// to t = fr + tl, whose rounding (2^-25 rev, 2e-7 rad) is an ABSOLUTE error of the angle: harmless for the embedded value, but a
// derivative factor cos(2^k x) or sin(2^k x) that sits near one of its zeros would carry it as a RELATIVE error of any size, and a
// per-point gradient -- unlike a sum over a ray's samples -- has nothing to hide it behind.  TwoSum keeps the lost part te and adds it
// back after the quadrant is removed (r is exact and small exactly where it matters): both factors are then accurate relative to
// their own magnitude.  Same reduction, same quadrant, same kernels; the value differs from sincos_rev's by at most that 2e-7.
SN_DEV void sincos_rev_comp(Rev2 p, float scale, float& s, float& c) {
  float th = p.hi * scale;                    // exact
  float tl = p.lo * scale;                    // exact
  float fr = th - __builtin_rintf(th);        // exact, in [-0.5, 0.5]
  float t = fr + tl;                          // rounded ...
  float bb = t - fr;
  float te = (fr - (t - bb)) + (tl - bb);     // ... and what the rounding lost (TwoSum: exact)
  float k = __builtin_rintf(t * 4.0f);        // quadrant -2..2
  float r = __builtin_fmaf(k, -0.25f, t) + te;   // the fma is exact: |r| <= 1/8 rev
  float a = r * 6.2831853071795864769f;       // radians, |a| <= pi/4
  float a2 = a * a;
  float sp = __builtin_fmaf(a2, -1.9515295891e-4f, 8.3321608736e-3f);
  sp = __builtin_fmaf(sp, a2, -1.6666654611e-1f);
  float sn = __builtin_fmaf(sp * a2, a, a);
  float cp = __builtin_fmaf(a2, 2.443315711809948e-5f, -1.388731625493765e-3f);
  cp = __builtin_fmaf(cp, a2, 4.166664568298827e-2f);
  float cs = __builtin_fmaf(cp * a2, a2, __builtin_fmaf(a2, -0.5f, 1.0f));
  int q = (int)k & 3;                          // two's complement: -1 -> 3, -2 -> 2
  float s1 = (q & 1) ? cs : sn;
  float c1 = (q & 1) ? sn : cs;
  s = (q & 2) ? -s1 : s1;
  c = ((q + 1) & 2) ? -c1 : c1;
}

template <int ROW>
__global__ void __launch_bounds__(WAVES * 64)
point_grad_kernel(const float* __restrict__ w1, const float* __restrict__ w5, const char* __restrict__ g_acts, long slot_rows,
                  const float* __restrict__ rays, const float* __restrict__ z_vals, long n_points, int S,
                  float* __restrict__ g_xyz) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lds_x = reinterpret_cast<float*>(smem);         // source 0 = W1 (k 0..255), source 1 = W5[:, 0:63]
  constexpr int NQ = RowTraits<ROW>::NQ;
  constexpr long RB = RowTraits<ROW>::ROW_BYTES;

  // ---- stage the weights once per workgroup: the LDS image of ray_grad_points_kernel's xyz part
  for (int idx = threadIdx.x; idx < 512 * 64; idx += WAVES * 64) {
    const int k = idx >> 6, f = idx & 63, tile = f >> 5, i = f & 31;
    const int col = xyz_col(row_half(i), 16 * tile + row_reg(i));
    float w = 0.0f;
    if (col >= 0) w = k < 256 ? w1[k * 63 + col] : w5[(k - 256) * 319 + col];
    lds_x[(k >> 8) * (256 * 64) + lds_pos<NQ>(k & 255, tile, 2, i)] = w;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5;
  const long n_tiles = (n_points + PTS_WG - 1) / PTS_WG;
  for (long tile_i = blockIdx.x; tile_i < n_tiles; tile_i += gridDim.x) {
    const long p = tile_i * PTS_WG + wave * 32 + (lane & 31);
    const long pl = p < n_points ? p : n_points - 1;     // rows >= n_points are never read; such a lane stores nothing
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    contract<ROW, 2, 256>(g_acts + (0 * slot_rows + pl) * RB, lds_x, lane, acc);
    contract<ROW, 2, 256>(g_acts + (4 * slot_rows + pl) * RB, lds_x + 256 * 64, lane, acc);

    // ---- embedding derivative (nerf.py:36-41) at xyz = o + d*z with separate roundings, the point the forward embedded
    const float* rp = rays + (pl / S) * 8;
    const float zz = z_vals[pl];
    const float x = __fadd_rn(rp[0], __fmul_rn(rp[3], zz)), y = __fadd_rn(rp[1], __fmul_rn(rp[4], zz)),
                z = __fadd_rn(rp[2], __fmul_rn(rp[5], zz));
    float gx[3] = {0.0f, 0.0f, 0.0f};
    const Rev2 px = to_revolutions(x), py = to_revolutions(y), pz = to_revolutions(z);
    const float hs = h ? 32.0f : 1.0f;                // bands 5..9 on the upper lane half
#pragma unroll
    for (int pp = 0; pp < 15; ++pp) {
      const Rev2 pc = (pp % 3 == 0) ? px : (pp % 3 == 1) ? py : pz;
      const float scale = hs * (float)(1 << (pp / 3));
      float s, c;
      sincos_rev_comp(pc, scale, s, c);
      const float g_sin = acc[(2 * pp) >> 4][(2 * pp) & 15], g_cos = acc[(2 * pp + 1) >> 4][(2 * pp + 1) & 15];
      gx[pp % 3] += scale * (c * g_sin - s * g_cos);
    }
    if (h) gx[2] += acc[1][14];                        // identity columns: x, y on the lower half, z on the upper
    else { gx[0] += acc[1][14]; gx[1] += acc[1][15]; }
    // the two lane halves hold disjoint bands of the same point
#pragma unroll
    for (int a = 0; a < 3; ++a) gx[a] += __shfl_xor(gx[a], 32, 64);
    if (h == 0 && p < n_points) {
      f32x4 out;
      out[0] = gx[0]; out[1] = gx[1]; out[2] = gx[2]; out[3] = 0.0f;
      *reinterpret_cast<f32x4*>(g_xyz + p * 4) = out;
    }
  }
}

__global__ void __launch_bounds__(256)
point_grad_wsum_kernel(const float* __restrict__ g_xyz, const float* __restrict__ weights, long n_rays, int S,
                       float* __restrict__ g_sum) {
  const int lane = threadIdx.x & 63;
  const long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;
  double a[3] = {0, 0, 0};
  const f32x4* src = reinterpret_cast<const f32x4*>(g_xyz + ray * (long)S * 4);
  const float* w = weights + ray * (long)S;
  for (int s = lane; s < S; s += 64) {
    const f32x4 g = src[s];
    const double ws = (double)w[s];
    a[0] += ws * (double)g[0]; a[1] += ws * (double)g[1]; a[2] += ws * (double)g[2];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = wave_sum(a[k]);
  if (lane == 0) {
    f32x4 out;
    out[0] = (float)a[0]; out[1] = (float)a[1]; out[2] = (float)a[2]; out[3] = 0.0f;
    *reinterpret_cast<f32x4*>(g_sum + ray * 4) = out;
  }
}

}  // namespace snrg

// layout: 0 = fp32 rows, 1 = bf16 rows, 2 = (hi, lo) pairs of the bf16x3 state
extern "C" int sn_point_grads_launch(const float* w1, const float* w5, int layout, const void* g_acts, long slot_rows,
                                     const float* rays, const float* z_vals, long n_rays, int n_samples, float* g_xyz,
                                     hipStream_t stream) {
  using namespace snrg;
  if (n_rays <= 0) return 0;
  const long n_points = n_rays * (long)n_samples;
  const long tiles = (n_points + PTS_WG - 1) / PTS_WG;
  const unsigned grid = snh::persistent_grid(tiles);
  constexpr size_t lds = LDS_FLOATS_XYZ * sizeof(float);
  const char* G = reinterpret_cast<const char*>(g_acts);
#define SN_PG(R)                                                                                                   \
  {                                                                                                                \
    SN_ENSURE_DYN_LDS((point_grad_kernel<R>), lds);                                                                \
    hipLaunchKernelGGL((point_grad_kernel<R>), dim3(grid), dim3(WAVES * 64), lds, stream, w1, w5, G, slot_rows,    \
                       rays, z_vals, n_points, n_samples, g_xyz);                                                  \
  }
  if (layout == 0) SN_PG(ROW_F32)
  else if (layout == 1) SN_PG(ROW_BF16)
  else SN_PG(ROW_X3)
#undef SN_PG
  return (int)hipGetLastError();
}

extern "C" int sn_point_grads_wsum_launch(const float* g_xyz, const float* weights, long n_rays, int n_samples, float* g_sum,
                                          hipStream_t stream) {
  if (n_rays <= 0) return 0;
  dim3 rays_grid;
  if (const int refused = snh::ray_grid(n_rays, &rays_grid)) return refused;
  hipLaunchKernelGGL(snrg::point_grad_wsum_kernel, rays_grid, dim3(256), 0, stream, g_xyz, weights, n_rays, n_samples, g_sum);
  return (int)hipGetLastError();
}
