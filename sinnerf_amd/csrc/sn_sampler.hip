// sn_sampler.hip -- the two device pieces of the one-image training sampler, gfx950 (the prose of both entries: include/sinnerf_hip.h):
//
//   valid_rows_kernel      one thread per (row y, x-origin): any of the pw mask bytes y, x0 + i sx -- lanes walk consecutive origins, so
//                          every load of a wave is one run of 64 consecutive bytes; thread 0 of block 0 clears n_valid
//   valid_cols_kernel      one thread per origin: any of the ph row results y0 + j sy, x0 (again consecutive bytes across a wave); the
//                          block's count goes to n_valid by ONE integer atomicAdd per block (ballot / popcount per wave, 4 words of LDS)
//   gather_windows_kernel  blockIdx.y = source; one thread per 32-bit word of its window, in channel-last order of the window
//
// pw + ph mask reads per origin instead of pw ph; the mask of a 400 x 400 frame is 160 kB and stays in L2 between the two passes.
// Integer sums only, so every output is the same on every call.  Nothing here allocates, synchronises or keeps state.
#include "sn_device.h"
#include "sn_launch.h"

namespace sns {

constexpr int MAX_SOURCES = 8;                    // == SN_GATHER_MAX_SOURCES of include/sinnerf_hip.h

struct GatherArgs {                               // passed by value: 8 x (8 + 8 + 4) + 4 = 164 bytes of kernel arguments
  const unsigned* src[MAX_SOURCES];
  unsigned* dst[MAX_SOURCES];
  int channels[MAX_SOURCES];
  unsigned planar_mask;
};

__global__ void __launch_bounds__(256)
valid_rows_kernel(const unsigned char* __restrict__ mask, int W, int stride_x, int patch_w, int nx, long n_rows_nx,
                  unsigned char* __restrict__ row_any, int* __restrict__ n_valid) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && n_valid != nullptr) *n_valid = 0;                 // ordered in front of valid_cols_kernel's atomics by the stream
  if (t >= n_rows_nx) return;
  const int y = (int)(t / nx), x0 = (int)(t - (long)y * nx);
  const unsigned char* row = mask + (long)y * W + x0;             // x0 + (patch_w - 1) stride_x <= W - 1: checked by the entry
  unsigned any = 0;
  for (int i = 0; i < patch_w; ++i) any |= row[(long)i * stride_x];
  row_any[t] = any != 0 ? 1 : 0;
}

__global__ void __launch_bounds__(256)
valid_cols_kernel(const unsigned char* __restrict__ row_any, int stride_y, int patch_h, int nx, long n_origins,
                  unsigned char* __restrict__ valid, int* __restrict__ n_valid) {
  __shared__ int sh[4];
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool set = false;
  if (t < n_origins) {
    const unsigned char* col = row_any + t;                       // row y0 of row_any starts at y0 nx, and t = y0 nx + x0
    unsigned any = 0;
    for (int j = 0; j < patch_h; ++j) any |= col[(long)j * stride_y * nx];   // y0 + (patch_h - 1) stride_y < the rows pass 1 wrote
    set = any != 0;
    valid[t] = set ? 1 : 0;
  }
  if (n_valid == nullptr) return;                                 // uniform over the grid
  const int c = __popcll(__ballot(set));                          // all 256 threads arrive: no early return above
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    if (total != 0) atomicAdd(n_valid, total);
  }
}

__global__ void __launch_bounds__(256)
gather_windows_kernel(const GatherArgs a, int H, int W, const int* __restrict__ origin, int stride_x, int stride_y, int patch_w,
                      int patch_h) {
  const int k = blockIdx.y;
  const int C = a.channels[k];
  const long n_pix = (long)patch_w * patch_h;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_pix * C) return;
  // the origin clamped into [0, W - (pw - 1) sx) x [0, H - (ph - 1) sy): both upper ends are >= 1 (checked by the entry), so every
  // source index below stays inside the frame whatever the two words hold
  const int max_x0 = W - 1 - (patch_w - 1) * stride_x, max_y0 = H - 1 - (patch_h - 1) * stride_y;
  const int x0 = min(max(origin[0], 0), max_x0), y0 = min(max(origin[1], 0), max_y0);
  const long p = e / C;
  const int c = (int)(e - p * C);
  const int iy = (int)(p / patch_w), ix = (int)(p - (long)iy * patch_w);
  const long s = ((long)(y0 + iy * stride_y) * W + (x0 + ix * stride_x)) * C + c;
  const long d = ((a.planar_mask >> k) & 1u) ? (long)c * n_pix + p : e;
  a.dst[k][d] = a.src[k][s];                                      // words, not floats: any bit pattern survives
}

}  // namespace sns

extern "C" long sn_valid_windows_workspace_bytes_impl(int H, int nx) { return (long)H * nx; }

extern "C" int sn_valid_windows_launch(const unsigned char* mask, int H, int W, int stride_x, int stride_y, int patch_w, int patch_h,
                                       int nx, int ny, unsigned char* valid, int* n_valid, void* workspace, hipStream_t stream) {
  using namespace sns;
  (void)H;
  unsigned char* row_any = reinterpret_cast<unsigned char*>(workspace);
  const long n_rows = (long)ny + (long)(patch_h - 1) * stride_y;          // the rows a candidate window reaches, <= H
  const long n1 = n_rows * nx, n2 = (long)ny * nx;
  hipLaunchKernelGGL(valid_rows_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, stream, mask, W, stride_x, patch_w, nx, n1,
                     row_any, n_valid);
  hipLaunchKernelGGL(valid_cols_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, stream, row_any, stride_y, patch_h, nx, n2,
                     valid, n_valid);
  return (int)hipGetLastError();
}

extern "C" int sn_gather_windows_launch(const void* const* src, void* const* dst, const int* channels, int n_src, unsigned planar_mask,
                                        int H, int W, const int* origin, int stride_x, int stride_y, int patch_w, int patch_h,
                                        hipStream_t stream) {
  using namespace sns;
  GatherArgs a = {};
  int c_max = 0;
  for (int k = 0; k < n_src; ++k) {
    a.src[k] = reinterpret_cast<const unsigned*>(src[k]);
    a.dst[k] = reinterpret_cast<unsigned*>(dst[k]);
    a.channels[k] = channels[k];
    c_max = channels[k] > c_max ? channels[k] : c_max;
  }
  a.planar_mask = planar_mask;
  const long n = (long)patch_w * patch_h * c_max;
  hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_src), dim3(256), 0, stream, a, H, W, origin,
                     stride_x, stride_y, patch_w, patch_h);
  return (int)hipGetLastError();
}
