// sn_warp.hip -- the forward warp of the reference view and its depth into the unseen view, and the draw of projected rays among the
// pixels that landed, gfx950 (the prose of both entries: include/sinnerf_hip.h):
//
//   warp_prepare_kernel    clears the keys; thread 0 of block 0 forms M = (src_proj ref_proj^-1)[:3, :] in fp64 (Gauss-Jordan)
//   warp_scatter_kernel    one thread per SOURCE pixel: project in fp64, clamp; per wave ONE 32-bit atomicMax or 64-bit atomicMin on the key
//                          of each distinct target (the lanes that share a target combine first)
//   warp_resolve_kernel    one thread per WINDOW pixel: decode the key, copy the winner's data row, recompute its depth
//   select_count_kernel / select_scan_kernel / select_pick_kernel      the k-th set element of a mask: block sums, their scan by one
//                          block, a binary search over blocks and a ballot / popcount walk inside the block -- integer sums, no atomics
//
// A key holds its winner whatever the order the atomics arrive in, so every output is deterministic.  Nothing here allocates, synchronises
// or reads a matrix on the host.
#include "sn_device.h"
#include "sn_launch.h"
#include "sn_wave.h"

namespace snw {

constexpr long WS_HEAD = 128;                     // bytes in front of the keys: M (12 doubles), padded
constexpr int SEL_CHUNK = 2048;                   // mask elements per block of select_count_kernel (256 threads x 8)
constexpr unsigned long long EMPTY64 = ~0ull;     // the cleared key of mode 1; as two 32-bit words it is the cleared key (-1) of mode 0

// fp32 bits in an order unsigned comparison preserves; -0.0 was folded onto +0.0 by the caller
SN_DEV unsigned ordered_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// p = M (x d, y d, d, 1), summed left to right
SN_DEV void project(const double* __restrict__ M, int x, int y, double d, double& p0, double& p1, double& p2) {
  const double xd = (double)x * d, yd = (double)y * d;
  p0 = ((M[0] * xd + M[1] * yd) + M[2] * d) + M[3];
  p1 = ((M[4] * xd + M[5] * yd) + M[6] * d) + M[7];
  p2 = ((M[8] * xd + M[9] * yd) + M[10] * d) + M[11];
}

__global__ void __launch_bounds__(256)
warp_prepare_kernel(const double* __restrict__ ref_proj, const double* __restrict__ src_proj, double* __restrict__ M,
                    unsigned long long* __restrict__ keys, long n_keys) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += (long)gridDim.x * blockDim.x) keys[i] = EMPTY64;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double a[4][8];                                 // [ref_proj | I] -> [I | ref_proj^-1], partial pivoting; a singular matrix gives inf / NaN
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { a[r][c] = ref_proj[r * 4 + c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
  for (int k = 0; k < 4; ++k) {
    int piv = k;
    for (int r = k + 1; r < 4; ++r)
      if (fabs(a[r][k]) > fabs(a[piv][k])) piv = r;
    for (int c = 0; c < 8; ++c) { const double t = a[k][c]; a[k][c] = a[piv][c]; a[piv][c] = t; }
    const double inv = 1.0 / a[k][k];
    for (int c = 0; c < 8; ++c) a[k][c] *= inv;
    for (int r = 0; r < 4; ++r) {
      if (r == k) continue;
      const double f = a[r][k];
      for (int c = 0; c < 8; ++c) a[r][c] -= f * a[k][c];
    }
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += src_proj[r * 4 + k] * a[k][4 + c];
      M[r * 4 + c] = s;
    }
}

__global__ void __launch_bounds__(256)
warp_scatter_kernel(const float* __restrict__ ref_depth, const double* __restrict__ M, int H, int W, double eps, int mode,
                    unsigned long long* __restrict__ keys) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool live = i < (long)H * W;                                        // no early return: the whole wave walks the loop below together
  long t = -1;
  unsigned long long key = EMPTY64;
  if (live) {
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    double p0, p1, p2;
    project(M, x, y, (double)ref_depth[i], p0, p1, p2);
    const double xs = p0 / (p2 + eps), ys = p1 / (p2 + eps);
    live = !(xs != xs || ys != ys);                                   // NaN: the source pixel is dropped
    // clamped in floating point, so +-inf and anything beyond int range end on a border before the conversion
    const int tx = (int)fmin(fmax(floor(xs), 0.0), (double)(W - 1)), ty = (int)fmin(fmax(floor(ys), 0.0), (double)(H - 1));
    t = (long)ty * W + tx;
    const float df = (float)p2 + 0.0f;                                // -0.0 -> +0.0: equal depths tie on the index
    key = ((unsigned long long)ordered_bits(df) << 32) | (unsigned long long)(unsigned)i;
  }
  // One atomic per DISTINCT target of the wave, not per lane.  The zero-depth background of a blender frame sends tens of thousands of
  // source pixels to one target, and that many atomics on one address take their turns (1.08 of the 1.44 ms of a 400 x 400 sampler
  // draw before this loop).  max and min are associative, so the key ends where the per-lane atomics left it.
  unsigned long long todo = __ballot(live);
  while (todo != 0ull) {                                              // wave-uniform: every lane sees the same ballot
    const int lead = __ffsll((long long)todo) - 1;
    const long t_lead = __shfl(t, lead, 64);
    const bool mine = live && t == t_lead;
    const unsigned long long group = __ballot(mine);
    if (mode == 0) {                                                  // the largest index of the group is its highest lane's
      if (lane == 63 - __clzll((long long)group)) atomicMax(reinterpret_cast<int*>(keys) + t, (int)i);
    } else if ((group & (group - 1ull)) == 0ull) {                    // a group of one
      if (mine) atomicMin(keys + t, key);
    } else {
      unsigned long long k = mine ? key : EMPTY64;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o, 64);
        k = other < k ? other : k;
      }
      if (lane == lead) atomicMin(keys + t, k);
    }
    todo &= ~group;
  }
}

__global__ void __launch_bounds__(256)
warp_resolve_kernel(const float* __restrict__ ref_depth, const unsigned* __restrict__ data, const double* __restrict__ M, int W, int C,
                    int mode, const unsigned long long* __restrict__ keys, int x0, int y0, int stride_x, int stride_y, int out_w,
                    long n_out, unsigned* __restrict__ out_new, float* __restrict__ new_depth, unsigned char* __restrict__ mask,
                    int* __restrict__ winner) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_out) return;
  const int iy = (int)(o / out_w), ix = (int)(o - (long)iy * out_w);
  const long t = (long)(y0 + iy * stride_y) * W + (x0 + ix * stride_x);
  int w;
  if (mode == 0) {
    w = reinterpret_cast<const int*>(keys)[t];
  } else {
    const unsigned long long k = keys[t];
    w = k == EMPTY64 ? -1 : (int)(unsigned)(k & 0xffffffffull);
  }
  if (winner != nullptr) winner[o] = w;
  if (mask != nullptr) mask[o] = w >= 0 ? 1 : 0;
  if (new_depth != nullptr) {
    float d = 0.0f;
    if (w >= 0) {
      const int sy = w / W, sx = w - sy * W;
      double p0, p1, p2;
      project(M, sx, sy, (double)ref_depth[w], p0, p1, p2);
      d = (float)p2;
    }
    new_depth[o] = d;
  }
  if (out_new != nullptr)
    for (int c = 0; c < C; ++c) out_new[o * C + c] = w >= 0 ? data[(long)w * C + c] : 0u;      // words, not floats: any bit pattern survives
}

// ---- k-th set element

__global__ void __launch_bounds__(256)
select_count_kernel(const unsigned char* __restrict__ mask, long n, int* __restrict__ sums) {
  __shared__ int sh[4];
  const long base = (long)blockIdx.x * SEL_CHUNK + (long)threadIdx.x * 8;
  int c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (base + k < n) c += mask[base + k] != 0;
  c = snwv::wave_sum(c);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one block: offs[b] = sums[0] + ... + sums[b - 1] for b <= n_blocks, so offs[n_blocks] = N
__global__ void __launch_bounds__(256)
select_scan_kernel(const int* __restrict__ sums, long n_blocks, int* __restrict__ offs, int* __restrict__ n_landed) {
  __shared__ int sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (long tile = 0; tile < n_blocks; tile += 256) {
    const long b = tile + threadIdx.x;
    const int v = b < n_blocks ? sums[b] : 0;
    const int incl = snwv::wave_incl_scan_add(v, lane);
    __syncthreads();                              // the previous tile's sh has been read
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wave; ++k) before += sh[k];
    if (b < n_blocks) offs[b] = carry + before + incl - v;
    carry += ((sh[0] + sh[1]) + sh[2]) + sh[3];
  }
  if (threadIdx.x == 0) {
    offs[n_blocks] = carry;
    if (n_landed != nullptr) *n_landed = carry;
  }
}

// one wave per sample
__global__ void __launch_bounds__(256)
select_pick_kernel(const unsigned char* __restrict__ mask, long n, const float* __restrict__ u, long m, const int* __restrict__ offs,
                   long n_blocks, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;                             // whole waves leave together
  const int N = offs[n_blocks];
  if (N <= 0) {
    if (lane == 0) idx[j] = -1;
    return;
  }
  const double t = floor((double)u[j] * (double)N);
  const int k = !(t >= 0.0) ? 0 : (t >= (double)N ? N - 1 : (int)t);        // u outside [0, 1) or NaN: clamped, no fault
  long lo = 0, hi = n_blocks - 1;                 // the last block b with offs[b] <= k; its count is positive because k < N
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= k) lo = mid; else hi = mid - 1;
  }
  int r = k - offs[lo];
  const long base = lo * SEL_CHUNK;
  for (int s = 0; s < SEL_CHUNK; s += 64) {
    const long e = base + s + lane;
    const bool set = e < n && mask[e] != 0;
    const unsigned long long b = __ballot(set);
    const int c = __popcll(b);
    if (r < c) {
      if (set && __popcll(b & ((1ull << lane) - 1ull)) == r) idx[j] = (int)e;
      return;
    }
    r -= c;
  }
}

static long sel_blocks(long n) { return (n + SEL_CHUNK - 1) / SEL_CHUNK; }

}  // namespace snw

extern "C" long sn_forward_warp_workspace_bytes_impl(int H, int W) { return snw::WS_HEAD + (long)H * W * 8; }

extern "C" int sn_forward_warp_launch(const float* ref_depth, const float* data, int H, int W, int C, const double* ref_proj,
                                      const double* src_proj, double eps, int mode, int x0, int y0, int stride_x, int stride_y,
                                      int out_w, int out_h, float* out_new, float* new_depth, unsigned char* mask, int* winner,
                                      void* workspace, hipStream_t stream) {
  using namespace snw;
  const long n = (long)H * W, n_out = (long)out_w * out_h;
  double* M = reinterpret_cast<double*>(workspace);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + WS_HEAD);
  const long n_keys = mode == 0 ? (n + 1) / 2 : n;                   // mode 0 uses the first 4 n bytes as 32-bit keys
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(warp_prepare_kernel, dim3(snh::stride_grid(n, 1024)), dim3(256), 0, stream, ref_proj, src_proj, M, keys,
                     n_keys);
  hipLaunchKernelGGL(warp_scatter_kernel, dim3(blocks), dim3(256), 0, stream, ref_depth, M, H, W, eps, mode, keys);
  hipLaunchKernelGGL(warp_resolve_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, stream, ref_depth,
                     reinterpret_cast<const unsigned*>(data), M, W, data != nullptr ? C : 0, mode, keys, x0, y0, stride_x, stride_y, out_w,
                     n_out, data != nullptr ? reinterpret_cast<unsigned*>(out_new) : nullptr, new_depth, mask, winner);
  return (int)hipGetLastError();
}

extern "C" long sn_select_landed_workspace_bytes_impl(long n) { return (2 * snw::sel_blocks(n) + 1) * (long)sizeof(int); }

extern "C" int sn_select_landed_launch(const unsigned char* mask, long n, const float* u, long m, int* idx, int* n_landed,
                                       void* workspace, hipStream_t stream) {
  using namespace snw;
  const long nb = sel_blocks(n);
  int* sums = reinterpret_cast<int*>(workspace);
  int* offs = sums + nb;
  hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)nb), dim3(256), 0, stream, mask, n, sums);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, stream, sums, nb, offs, n_landed);
  if (m > 0)
    hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, mask, n, u, m, offs, nb, idx);
  return (int)hipGetLastError();
}
