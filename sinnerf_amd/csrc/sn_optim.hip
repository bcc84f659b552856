// sn_optim.hip -- the reference's optimisers over ONE flat fp32 parameter / gradient buffer (the all-reduce buffer), gfx950:
//   adam_kernel     utils/__init__.py:19-21 (torch.optim.Adam, eps=1e-8); in namespace snx, the name the traces and profiles know it by
//   sgd_kernel      utils/__init__.py:16-18 (torch.optim.SGD: momentum, dampening 0, no Nesterov, weight decay folded into the gradient)
//   radam_kernel    utils/optimizers.py:62-104 (RAdam) and :393-437 (Ranger = the same moments and update + lookahead), the element-wise part
// one launch per step, in place.  The per-step scalars of the last two -- N_sma, the rectified / degenerate step size, their
// products with the learning rate, whether the lookahead fires -- are computed by the caller in double from the HOST step counter and
// arrive rounded to fp32 once, as torch rounds a Python scalar; nothing is read back from the device.
//
// HBM-bound element-wise work: lane i of a wave at float4 i (16 B per lane, 1 KiB per wave instruction) over the first n/4*4 elements when
// every buffer is 16-byte aligned, the remaining n%4 (or all n, for unaligned buffers) one float per lane.  The arithmetic is plain C++
// under -ffp-contract=off: one rounding per operation, in the reference's order.
#include "sn_device.h"
#include "sn_launch.h"

namespace snx {

// torch.optim.Adam (amsgrad=False, maximize=False), weight_decay folded in L2 style like torch:
//   g += wd*p ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
            float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
  const float step_size = lr / bc1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float gi = g[i];
    const float pi = p[i];
    if (wd != 0.0f) gi = gi + wd * pi;
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

}  // namespace snx

namespace sno {

// g += wd p ; buf = momentum buf + g ; p -= lr buf           (buf = g without momentum; a zeroed buffer gives torch's first step buf = g)
struct SgdArgs { float lr, momentum, wd; };
template <bool MOMENTUM>
SN_DEV void sgd_update(float& p, float g, float& buf, const SgdArgs& a) {
  if (a.wd != 0.0f) g = g + a.wd * p;
  if (MOMENTUM) { buf = buf * a.momentum + g; g = buf; }
  p = p + (-a.lr) * g;
}

template <bool MOMENTUM>
__global__ void __launch_bounds__(256)
sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n4, long n, SgdArgs a) {
  const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* b4 = reinterpret_cast<float4*>(buf);
  for (long i = t0; i < n4; i += stride) {
    float4 pv = p4[i], bv = MOMENTUM ? b4[i] : float4{0.0f, 0.0f, 0.0f, 0.0f};
    const float4 gv = g4[i];
    sgd_update<MOMENTUM>(pv.x, gv.x, bv.x, a); sgd_update<MOMENTUM>(pv.y, gv.y, bv.y, a);
    sgd_update<MOMENTUM>(pv.z, gv.z, bv.z, a); sgd_update<MOMENTUM>(pv.w, gv.w, bv.w, a);
    if (MOMENTUM) b4[i] = bv;
    p4[i] = pv;
  }
  for (long i = 4 * n4 + t0; i < n; i += stride) {
    float pi = p[i], bi = MOMENTUM ? buf[i] : 0.0f;
    sgd_update<MOMENTUM>(pi, g[i], bi, a);
    if (MOMENTUM) buf[i] = bi;
    p[i] = pi;
  }
}

// v = v b2 + (1-b2) g g ; m = m b1 + (1-b1) g ; [p -= decay p] ; p -= coeff (m / (sqrt(v) + eps)  |  m) ; [slow += alpha (p - slow) ; p = slow]
//   update == 0: the moments only (RAdam with degenerated_to_sgd=False below the threshold: no decay either, optimizers.py:99-104)
struct RadamArgs { float b1, b2, omb1, omb2, eps, decay, coeff, alpha; int rectified, update; };
template <bool LOOKAHEAD>
SN_DEV void radam_update(float& p, float g, float& m, float& v, float& slow, const RadamArgs& a) {
  v = v * a.b2 + a.omb2 * g * g;
  m = m * a.b1 + a.omb1 * g;
  if (!a.update) return;
  if (a.decay != 0.0f) p = p + (-a.decay) * p;
  if (a.rectified) {
    const float denom = sqrtf(v) + a.eps;
    p = p + ((-a.coeff) * m) / denom;
  } else {
    p = p + (-a.coeff) * m;
  }
  if (LOOKAHEAD) {
    slow = slow + a.alpha * (p - slow);
    p = slow;
  }
}

template <bool LOOKAHEAD>
__global__ void __launch_bounds__(256)
radam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ slow,
             long n4, long n, RadamArgs a) {
  const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  float4* s4 = reinterpret_cast<float4*>(slow);
  for (long i = t0; i < n4; i += stride) {
    float4 pv = p4[i], mv = m4[i], vv = v4[i], sv = LOOKAHEAD ? s4[i] : float4{0.0f, 0.0f, 0.0f, 0.0f};
    const float4 gv = g4[i];
    radam_update<LOOKAHEAD>(pv.x, gv.x, mv.x, vv.x, sv.x, a); radam_update<LOOKAHEAD>(pv.y, gv.y, mv.y, vv.y, sv.y, a);
    radam_update<LOOKAHEAD>(pv.z, gv.z, mv.z, vv.z, sv.z, a); radam_update<LOOKAHEAD>(pv.w, gv.w, mv.w, vv.w, sv.w, a);
    m4[i] = mv; v4[i] = vv;
    if (a.update) p4[i] = pv;
    if (LOOKAHEAD) s4[i] = sv;
  }
  for (long i = 4 * n4 + t0; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i], si = LOOKAHEAD ? slow[i] : 0.0f;
    radam_update<LOOKAHEAD>(pi, g[i], mi, vi, si, a);
    m[i] = mi; v[i] = vi;
    if (a.update) p[i] = pi;
    if (LOOKAHEAD) slow[i] = si;
  }
}

inline bool aligned16(const void* q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// grid-stride, 256 threads, at most 4096 blocks (adam_kernel's shape), counted in the units a thread handles
inline unsigned grid_for(long n4, long n) { return snh::stride_grid_min1(n4 > 0 ? n4 : n, 4096); }

}  // namespace sno

extern "C" int sn_adam_step_launch(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                                   float eps, float wd, int step, hipStream_t stream) {
  if (n <= 0) return 0;
  const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
  hipLaunchKernelGGL(snx::adam_kernel, dim3(snh::stride_grid(n, 4096)), dim3(256), 0, stream, p, g, m, v, n, lr, b1, b2, eps, wd,
                     (float)bc1, (float)sqrt(bc2));
  return (int)hipGetLastError();
}

extern "C" int sn_sgd_step_launch(float* p, const float* g, float* buf, long n, double lr, double momentum, double wd, hipStream_t stream) {
  using namespace sno;
  if (n <= 0) return 0;
  const bool mom = momentum != 0.0;
  const long n4 = (aligned16(p) && aligned16(g) && (!mom || aligned16(buf))) ? n / 4 : 0;
  const SgdArgs a = {(float)lr, (float)momentum, (float)wd};
  const unsigned blocks = grid_for(n4, n);
  if (mom) hipLaunchKernelGGL(sgd_kernel<true>, dim3(blocks), dim3(256), 0, stream, p, g, buf, n4, n, a);
  else hipLaunchKernelGGL(sgd_kernel<false>, dim3(blocks), dim3(256), 0, stream, p, g, (float*)nullptr, n4, n, a);
  return (int)hipGetLastError();
}

// slow == nullptr: RAdam (step_coeff < 0 = no parameter update); otherwise Ranger (lookahead when sync != 0)
extern "C" int sn_radam_step_launch(float* p, const float* g, float* m, float* v, long n, double b1, double b2, double eps, double decay,
                                    double step_coeff, int rectified, float* slow, double alpha, int sync, hipStream_t stream) {
  using namespace sno;
  if (n <= 0) return 0;
  const bool look = slow != nullptr && sync != 0;
  const long n4 = (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!look || aligned16(slow))) ? n / 4 : 0;
  RadamArgs a;
  a.b1 = (float)b1; a.b2 = (float)b2; a.omb1 = (float)(1.0 - b1); a.omb2 = (float)(1.0 - b2);
  a.eps = (float)eps; a.decay = (float)decay; a.coeff = (float)step_coeff; a.alpha = (float)alpha;
  a.rectified = rectified != 0; a.update = !(step_coeff < 0.0);
  const unsigned blocks = grid_for(n4, n);
  if (look) hipLaunchKernelGGL(radam_kernel<true>, dim3(blocks), dim3(256), 0, stream, p, g, m, v, slow, n4, n, a);
  else hipLaunchKernelGGL(radam_kernel<false>, dim3(blocks), dim3(256), 0, stream, p, g, m, v, (float*)nullptr, n4, n, a);
  return (int)hipGetLastError();
}
