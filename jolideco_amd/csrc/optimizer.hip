// The stand-alone optimizer step (gfx950): every kernel that steps a parameter outside a prior's own last kernel, and the six
// C entries that launch them.  Chain rule, update and new flux in one pass, 16 B per lane where every image is 16-byte
// aligned, a scalar kernel otherwise, the bias terms by value or from device memory.  Two kernels, one launcher each:
// optimizer_kernel (an image; jd_adam_step, jd_adam_step_addends, jd_sgd_step, jd_optimizer_step) and
// optimizer_multi_kernel (up to 64 small vectors; jd_adam_step_multi, jd_optimizer_step_multi).  The KIND of an
// instantiation says what is compiled in: the plain kinds are adam_update (jd_adam.h) in float32 and nothing else -- the
// bits of the fused steps of gmm_gather.hip -- and the options of torch.optim.Adam / torch.optim.SGD (weight decay,
// decoupled weight decay, AMSGrad; weight decay, momentum, dampening, Nesterov) are kinds of their own: Adam's few
// operations per parameter in double (adam_update_wide below), SGD's in torch's own float32 order.
// Bytes per pixel (log flux, no mask): Adam 36 (theta, flux, grad, m, v in; theta, flux, m, v out), + 4 per addend image,
// + amsgrad 44; SGD 20, + momentum 28 (first step 24: the buffer is only written).
#include <cmath>
#include <cstdint>

#include "jd_common.h"
#include "kernels.h"
#include "jd_adam.h"

namespace jd {

constexpr int OPT_BLOCK = 256;
constexpr int OPT_MAX_BLOCKS = 4096;  // grid cap of the grid-stride loops
// what a kernel instantiation compiles in: the update (float32 adam_update for OPT_ADAM and OPT_SGD, double for
// OPT_ADAM_DECAY and OPT_AMSGRAD -- the plain kinds hold no double arithmetic and no register for it) and the state images
// it keeps in registers beside theta
enum { OPT_ADAM = 0, OPT_ADAM_DECAY = 1, OPT_AMSGRAD = 2, OPT_SGD = 3, OPT_MOMENTUM = 4 };
constexpr bool opt_moments(int kind) { return kind == OPT_ADAM || kind == OPT_ADAM_DECAY || kind == OPT_AMSGRAD; }
constexpr bool opt_third(int kind) { return kind == OPT_AMSGRAD || kind == OPT_MOMENTUM; }

struct OptTerms {  // uniform terms of the options (the Adam terms of the plain update travel in AdamArgs)
  float weight_decay;         // 0: none
  float decay;                // fp32(1 - lr * weight_decay), decoupled
  float momentum;             // SGD
  float one_minus_dampening;  // fp32(1 - dampening)
  int decoupled, nesterov;
};

struct OptArgs {
  AdamArgs a;   // images, n, the terms of the plain update, zero_grad, sgd, linear, bias_dev, addend (OPT_ADAM only)
  float* s;     // OPT_AMSGRAD: max_exp_avg_sq; OPT_MOMENTUM: momentum_buffer
  OptTerms t;
  int first_step;
};

// Adam with an option: the handful of operations of one parameter in DOUBLE, every stored quantity rounded to float32
// once.  The tests hold a step to torch.optim in float64 under 4 x the error of torch.optim in float32, per pixel for the
// flux -- and the flux of a LINEAR parameter whose step lands next to zero is the rounding error of the update over a
// value a thousand times smaller: which float32 implementation is the unlucky one there is a matter of operation order
// (torch's own float32 kernels differ from host to host in 2 % of the parameters; adam_update's order, torch's order on
// one host and on another each missed the bound in a few of 128 cases and met it in the others).  In double the error
// left is that of the float32 images themselves, whatever the order.  The kernel stays bound by HBM: one double square
// root and two double divisions per parameter beside 36 to 44 bytes of traffic.
template <bool AMSGRAD>
__device__ __forceinline__ void adam_update_wide(float& th, float& m, float& v, float& s, float g, const AdamArgs& a,
                                                 const OptTerms& t) {
#pragma clang fp contract(off)
  double thd = th, gd = g;
  if (t.weight_decay != 0.f) {
    if (t.decoupled)
      thd = thd * (double)t.decay;  // param.mul_(1 - lr * weight_decay)
    else
      gd = gd + (double)t.weight_decay * thd;  // grad.add(param, alpha=weight_decay)
  }
  const double md = (double)m + (double)a.one_minus_beta1 * (gd - (double)m);
  const double vd = (double)v * (double)a.beta2 + (double)a.one_minus_beta2 * (gd * gd);
  double second = vd;
  if constexpr (AMSGRAD) {
    second = fmax((double)s, vd);  // torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)
    s = (float)second;
  }
  const double denom = sqrt(second) / (double)a.bias2_sqrt + (double)a.eps;
  th = (float)(thd - (double)a.step_size * (md / denom));
  m = (float)md, v = (float)vd;
}

// One parameter: th, the moments m / v and the third state s (max_exp_avg_sq or the momentum buffer) are updated in place.
// OPT_ADAM, and OPT_SGD without weight decay, ARE adam_update (jd_adam.h): the bits of the fused kernels.
// SGD with options follows torch's float32 CPU kernels operation by operation -- add(x, alpha=c) is one multiply-add, as
// jd_adam.h found for the plain step -- and gives their bits; explicit fmaf and `fp contract(off)` keep every path the same
// in every kernel: optimizer_multi_kernel must give the bits of optimizer_kernel.
template <int KIND>
__device__ __forceinline__ void opt_update(float& th, float& m, float& v, float& s, float g, const AdamArgs& a,
                                           const OptTerms& t, int first_step) {
#pragma clang fp contract(off)
  if constexpr (KIND == OPT_AMSGRAD) {
    adam_update_wide<true>(th, m, v, s, g, a, t);
  } else if constexpr (KIND == OPT_ADAM_DECAY) {
    adam_update_wide<false>(th, m, v, s, g, a, t);
  } else if constexpr (KIND == OPT_ADAM) {
    adam_update(th, m, v, g, a);
  } else {
    if (t.weight_decay != 0.f) g = fmaf(t.weight_decay, th, g);  // grad.add(param, alpha=weight_decay)
    if constexpr (KIND == OPT_SGD) {
      adam_update(th, m, v, g, a);  // (a.sgd: param.add_(grad, alpha=-lr))
    } else {
      // buf = grad (first step) | buf.mul_(momentum).add_(grad, alpha=1 - dampening)
      s = first_step ? g : fmaf(t.one_minus_dampening, g, s * t.momentum);
      g = t.nesterov ? fmaf(t.momentum, s, g) : s;  // grad.add(buf, alpha=momentum) | buf
      th = fmaf(-a.lr, g, th);                      // param.add_(grad, alpha=-lr)
    }
  }
}

// chain rule + update + new flux of one pixel: adam_pixel (jd_adam.h, the fused kernels' form) with the third state image
template <int KIND>
__device__ __forceinline__ void opt_pixel(float& th, float& f, float& m, float& v, float& s, float gf, float mk,
                                          const OptArgs& o) {
  const AdamArgs& a = o.a;
  const float dfdth = a.linear ? (a.mask ? mk : 1.f) : f;
  opt_update<KIND>(th, m, v, s, gf * dfdth, a, o.t, o.first_step);
  f = a.linear ? th : expf(th);
  if (a.mask) f *= mk;
}

__device__ __forceinline__ void unpack(const float4 q, float (&x)[4]) { x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w; }

// NA: addend images (a.addend[0 .. NA) are set), added to the gradient in order before the update (jd_adam.h)
template <int VEC, int KIND, int NA>
__global__ __launch_bounds__(OPT_BLOCK) void optimizer_kernel(OptArgs o) {
  static_assert(NA == 0 || KIND == OPT_ADAM, "only the plain Adam step takes addend images (jd_adam_step_addends)");
  constexpr bool MOMENTS = opt_moments(KIND), THIRD = opt_third(KIND);
  use_device_bias(o.a);
  const AdamArgs& a = o.a;
  // (the first step of a momentum buffer writes it without reading it)
  const bool read_third = KIND == OPT_AMSGRAD || (KIND == OPT_MOMENTUM && !o.first_step);
  const size_t stride = (size_t)gridDim.x * OPT_BLOCK * VEC;
  for (size_t i = ((size_t)blockIdx.x * OPT_BLOCK + threadIdx.x) * VEC; i < a.n; i += stride) {
    float th[VEC], f[VEC], gf[VEC], m[VEC], v[VEC], s[VEC], mk[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) m[k] = v[k] = s[k] = 0.f, mk[k] = 1.f;
    if constexpr (VEC == 4) {
      unpack(*reinterpret_cast<const float4*>(a.theta + i), th);
      unpack(*reinterpret_cast<const float4*>(a.flux_in + i), f);
      unpack(*reinterpret_cast<const float4*>(a.grad_flux + i), gf);
      float4 a4[NA ? NA : 1];
#pragma unroll
      for (int k = 0; k < NA; ++k) a4[k] = *reinterpret_cast<const float4*>(a.addend[k] + i);
      if constexpr (MOMENTS) {
        unpack(*reinterpret_cast<const float4*>(a.m + i), m);
        unpack(*reinterpret_cast<const float4*>(a.v + i), v);
      }
      if constexpr (THIRD)
        if (read_third) unpack(*reinterpret_cast<const float4*>(o.s + i), s);
      if (a.mask) unpack(*reinterpret_cast<const float4*>(a.mask + i), mk);
#pragma unroll
      for (int k = 0; k < NA; ++k) gf[0] += a4[k].x, gf[1] += a4[k].y, gf[2] += a4[k].z, gf[3] += a4[k].w;
    } else {
      th[0] = a.theta[i], f[0] = a.flux_in[i], gf[0] = a.grad_flux[i];
#pragma unroll
      for (int k = 0; k < NA; ++k) gf[0] += a.addend[k][i];
      if constexpr (MOMENTS) m[0] = a.m[i], v[0] = a.v[i];
      if constexpr (THIRD)
        if (read_third) s[0] = o.s[i];
      if (a.mask) mk[0] = a.mask[i];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) opt_pixel<KIND>(th[k], f[k], m[k], v[k], s[k], gf[k], mk[k], o);
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(a.theta + i) = make_float4(th[0], th[1], th[2], th[3]);
      *reinterpret_cast<float4*>(a.flux_out + i) = make_float4(f[0], f[1], f[2], f[3]);
      if constexpr (MOMENTS) {
        *reinterpret_cast<float4*>(a.m + i) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4*>(a.v + i) = make_float4(v[0], v[1], v[2], v[3]);
      }
      if constexpr (THIRD) *reinterpret_cast<float4*>(o.s + i) = make_float4(s[0], s[1], s[2], s[3]);
      if (a.zero_grad) *reinterpret_cast<float4*>(a.grad_flux + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      a.theta[i] = th[0], a.flux_out[i] = f[0];
      if constexpr (MOMENTS) a.m[i] = m[0], a.v[i] = v[0];
      if constexpr (THIRD) o.s[i] = s[0];
      if (a.zero_grad) a.grad_flux[i] = 0.f;
    }
  }
}

// MANY small parameter vectors in one launch (the calibration parameters of the datasets of a joint step: two tensors of 2
// and 1 floats per dataset -- one launch each took 4.5 us, sixteen per step of eight observations; the source vectors of a
// sparse component).  One block per tensor, the update of optimizer_kernel with use_log_flux = 0 and no mask (opt_update:
// the same device function, the same bits).
constexpr int OPT_MULTI_MAX = 64;
struct OptMultiArgs {  // (3.4 KB of the 4 KB a kernel's arguments may take)
  float* theta[OPT_MULTI_MAX];
  const float* grad[OPT_MULTI_MAX];
  float* m[OPT_MULTI_MAX];
  float* v[OPT_MULTI_MAX];
  float* s[OPT_MULTI_MAX];
  int size[OPT_MULTI_MAX];
  float step_size[OPT_MULTI_MAX], bias2_sqrt[OPT_MULTI_MAX];
  unsigned long long first_step;  // bit i: tensor i takes its first momentum step
  float beta1, beta2, one_minus_beta1, one_minus_beta2, eps, lr;
  OptTerms t;
  const float* bias_dev;  // nullable, device [2 n]: {step_size, bias2_sqrt} of tensor i at [2 i]
};

template <int KIND>
__global__ __launch_bounds__(64) void optimizer_multi_kernel(OptMultiArgs a) {
  constexpr bool MOMENTS = opt_moments(KIND), THIRD = opt_third(KIND);
  float* theta = nullptr;
  const float* grad = nullptr;
  float *m = nullptr, *v = nullptr, *s = nullptr;
  int size = 0;
  AdamArgs p{};
  p.beta1 = a.beta1, p.beta2 = a.beta2, p.one_minus_beta1 = a.one_minus_beta1, p.one_minus_beta2 = a.one_minus_beta2;
  p.eps = a.eps, p.lr = a.lr, p.sgd = (KIND == OPT_SGD || KIND == OPT_MOMENTUM) ? 1 : 0;
  // (compile-time indices: indexing the by-value argument arrays with blockIdx would send them through scratch memory;
  // in groups of eight behind a uniform branch, so that no variant holds all 64 entries of an array in SGPRs at once)
#pragma unroll
  for (int g = 0; g < OPT_MULTI_MAX; g += 8)
    if ((int)(blockIdx.x & ~7u) == g)
#pragma unroll
      for (int i = g; i < g + 8; ++i)
        if ((int)blockIdx.x == i) {
          theta = a.theta[i], grad = a.grad[i], size = a.size[i];
          if constexpr (MOMENTS) m = a.m[i], v = a.v[i], p.step_size = a.step_size[i], p.bias2_sqrt = a.bias2_sqrt[i];
          if constexpr (THIRD) s = a.s[i];
        }
  if (MOMENTS && a.bias_dev) p.step_size = a.bias_dev[2 * blockIdx.x], p.bias2_sqrt = a.bias_dev[2 * blockIdx.x + 1];
  const int first = (int)((a.first_step >> blockIdx.x) & 1ull);
  for (int j = threadIdx.x; j < size; j += 64) {
    float th = theta[j], mj = 0.f, vj = 0.f, sj = 0.f;
    if constexpr (MOMENTS) mj = m[j], vj = v[j];
    if constexpr (KIND == OPT_AMSGRAD) sj = s[j];
    if constexpr (KIND == OPT_MOMENTUM)
      if (!first) sj = s[j];
    opt_update<KIND>(th, mj, vj, sj, grad[j], p, a.t, first);
    theta[j] = th;
    if constexpr (MOMENTS) m[j] = mj, v[j] = vj;
    if constexpr (THIRD) s[j] = sj;
  }
}

// the refusals both entries share; fills the kernel variant and the uniform terms
static int read_options(const jd_optimizer_options* opt, const char* who, int& kind, OptTerms& t) {
  JD_REQUIRE(opt, "%s: null options", who);
  JD_REQUIRE(opt->kind == JD_OPTIMIZER_ADAM || opt->kind == JD_OPTIMIZER_SGD, "%s: unknown optimizer kind %d", who, opt->kind);
  auto ok = [](double x) { return x >= 0.0 && std::isfinite(x); };
  // (torch.optim.SGD takes any dampening, a negative one too)
  JD_REQUIRE(ok(opt->lr) && ok(opt->weight_decay) && ok(opt->momentum) && std::isfinite(opt->dampening),
             "%s: lr, weight_decay and momentum must be finite and >= 0, dampening finite", who);
  const bool adam = opt->kind == JD_OPTIMIZER_ADAM;
  if (adam) {
    JD_REQUIRE(opt->momentum == 0.0 && opt->dampening == 0.0 && !opt->nesterov,
               "%s: momentum, dampening and nesterov are options of SGD", who);
  } else {
    JD_REQUIRE(!opt->amsgrad && !opt->decoupled_weight_decay, "%s: amsgrad and decoupled_weight_decay are options of Adam", who);
    JD_REQUIRE(!opt->nesterov || (opt->momentum > 0.0 && opt->dampening == 0.0),
               "%s: nesterov needs a momentum and zero dampening", who);
  }
  t.weight_decay = (float)opt->weight_decay;
  if (adam)
    kind = opt->amsgrad ? OPT_AMSGRAD : (t.weight_decay != 0.f ? OPT_ADAM_DECAY : OPT_ADAM);
  else
    kind = opt->momentum != 0.0 ? OPT_MOMENTUM : OPT_SGD;
  t.decoupled = opt->decoupled_weight_decay ? 1 : 0;
  t.decay = (float)(1.0 - opt->lr * opt->weight_decay);
  t.momentum = (float)opt->momentum;
  t.one_minus_dampening = (float)(1.0 - opt->dampening);
  t.nesterov = opt->nesterov ? 1 : 0;
  return JD_OK;
}

template <int KIND, int NA = 0>
static void launch_optimizer_kernel(bool vec, unsigned blocks, const OptArgs& o, hipStream_t stream) {
  if (vec)
    optimizer_kernel<4, KIND, NA><<<blocks, OPT_BLOCK, 0, stream>>>(o);
  else
    optimizer_kernel<1, KIND, NA><<<blocks, OPT_BLOCK, 0, stream>>>(o);
}

// The launcher of every stand-alone step of an image: `o` is filled (o.s and the state images a kind does not use are null).
static int launch_step(int kind, const OptArgs& o, hipStream_t stream) {
  const AdamArgs& a = o.a;
  int na = 0;
  while (na < ADDEND_MAX && a.addend[na]) ++na;
  // float4 accesses: every image the kernel touches is 16-byte aligned (null images count as aligned), else pixel by pixel
  bool vec = (a.n % 4 == 0) && aligned16(a.theta) && aligned16(a.flux_in) && aligned16(a.flux_out) && aligned16(a.grad_flux) &&
             aligned16(a.m) && aligned16(a.v) && aligned16(o.s) && aligned16(a.mask);
  for (int k = 0; k < na; ++k) vec = vec && aligned16(a.addend[k]);
  const size_t per_block = (size_t)OPT_BLOCK * (vec ? 4 : 1);
  size_t count = (a.n + per_block - 1) / per_block;
  if (count > OPT_MAX_BLOCKS) count = OPT_MAX_BLOCKS;
  const unsigned blocks = (unsigned)count;
  ProfScope prof(JD_KERNEL_ADAM, stream);
  switch (kind) {
    case OPT_ADAM:
      switch (na) {
        case 0: launch_optimizer_kernel<OPT_ADAM, 0>(vec, blocks, o, stream); break;
        case 1: launch_optimizer_kernel<OPT_ADAM, 1>(vec, blocks, o, stream); break;
        case 2: launch_optimizer_kernel<OPT_ADAM, 2>(vec, blocks, o, stream); break;
        case 3: launch_optimizer_kernel<OPT_ADAM, 3>(vec, blocks, o, stream); break;
        default: launch_optimizer_kernel<OPT_ADAM, 4>(vec, blocks, o, stream); break;
      }
      break;
    case OPT_ADAM_DECAY: launch_optimizer_kernel<OPT_ADAM_DECAY>(vec, blocks, o, stream); break;
    case OPT_AMSGRAD: launch_optimizer_kernel<OPT_AMSGRAD>(vec, blocks, o, stream); break;
    case OPT_SGD: launch_optimizer_kernel<OPT_SGD>(vec, blocks, o, stream); break;
    default: launch_optimizer_kernel<OPT_MOMENTUM>(vec, blocks, o, stream); break;
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// The launcher of every step of many small vectors: one block per tensor.
static int launch_step_multi(int kind, int n_tensors, const OptMultiArgs& a, hipStream_t stream) {
  ProfScope prof(JD_KERNEL_ADAM, stream);
  switch (kind) {
    case OPT_ADAM: optimizer_multi_kernel<OPT_ADAM><<<n_tensors, 64, 0, stream>>>(a); break;
    case OPT_ADAM_DECAY: optimizer_multi_kernel<OPT_ADAM_DECAY><<<n_tensors, 64, 0, stream>>>(a); break;
    case OPT_AMSGRAD: optimizer_multi_kernel<OPT_AMSGRAD><<<n_tensors, 64, 0, stream>>>(a); break;
    case OPT_SGD: optimizer_multi_kernel<OPT_SGD><<<n_tensors, 64, 0, stream>>>(a); break;
    default: optimizer_multi_kernel<OPT_MOMENTUM><<<n_tensors, 64, 0, stream>>>(a); break;
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd

using namespace jd;

extern "C" int jd_optimizer_step(float* theta, const float* flux_in, float* flux_out, float* grad_flux, float* exp_avg,
                                 float* exp_avg_sq, float* max_exp_avg_sq, float* momentum_buffer, const float* mask,
                                 size_t n, const jd_optimizer_options* options, int zero_grad, int use_log_flux,
                                 const float* bias_dev, void* stream) {
  JD_REQUIRE(theta && flux_in && flux_out && grad_flux && n > 0, "jd_optimizer_step: null argument or n == 0");
  int kind = 0;
  OptArgs o{};
  if (int status = read_options(options, "jd_optimizer_step", kind, o.t)) return status;
  const bool adam = opt_moments(kind);
  JD_REQUIRE(!adam || (exp_avg && exp_avg_sq), "jd_optimizer_step: Adam needs its moment images");
  JD_REQUIRE(kind != OPT_AMSGRAD || max_exp_avg_sq, "jd_optimizer_step: amsgrad needs max_exp_avg_sq");
  JD_REQUIRE(kind != OPT_MOMENTUM || momentum_buffer, "jd_optimizer_step: momentum needs momentum_buffer");
  AdamArgs& a = o.a;
  a.theta = theta, a.flux_in = flux_in, a.flux_out = flux_out, a.grad_flux = grad_flux, a.mask = mask, a.n = n;
  a.zero_grad = zero_grad, a.linear = use_log_flux ? 0 : 1;
  if (adam) {
    a.m = exp_avg, a.v = exp_avg_sq;
    a.step_size = options->step_size, a.beta1 = options->beta1, a.beta2 = options->beta2;
    a.one_minus_beta1 = options->one_minus_beta1, a.one_minus_beta2 = options->one_minus_beta2;
    a.bias2_sqrt = options->bias2_sqrt, a.eps = options->eps, a.bias_dev = bias_dev;
  } else {
    a.sgd = 1, a.bias2_sqrt = 1.f, a.lr = (float)options->lr;
  }
  o.s = kind == OPT_AMSGRAD ? max_exp_avg_sq : (kind == OPT_MOMENTUM ? momentum_buffer : nullptr);
  o.first_step = (kind == OPT_MOMENTUM && options->first_step) ? 1 : 0;
  return launch_step(kind, o, as_stream(stream));
}

extern "C" int jd_adam_step_addends(float* theta, const float* flux_in, float* flux_out, float* grad_flux,
                                    float* exp_avg, float* exp_avg_sq, const float* mask, size_t n, float step_size,
                                    float beta1, float beta2, float one_minus_beta1, float one_minus_beta2,
                                    float bias2_sqrt, float eps, int zero_grad, int use_log_flux, const float* bias_dev,
                                    const float* const* addends, void* stream) {
  JD_REQUIRE(theta && flux_in && flux_out && grad_flux && exp_avg && exp_avg_sq && n > 0,
             "jd_adam_step: null argument or n == 0");
  OptArgs o{};
  o.a = AdamArgs{theta, flux_in, flux_out, grad_flux, exp_avg, exp_avg_sq, mask, n,
                 step_size, beta1, beta2, one_minus_beta1, one_minus_beta2, bias2_sqrt, eps, 0.f, zero_grad, 0,
                 use_log_flux ? 0 : 1, bias_dev};
  static_assert(ADDEND_MAX == JD_ADDEND_MAX, "the host array of jd_adam_step_addends and AdamArgs::addend");
  for (int k = 0; addends && k < ADDEND_MAX && addends[k]; ++k) o.a.addend[k] = addends[k];  // (the leading non-null entries)
  return launch_step(OPT_ADAM, o, as_stream(stream));
}

extern "C" int jd_adam_step(float* theta, const float* flux_in, float* flux_out, float* grad_flux,
                            float* exp_avg, float* exp_avg_sq, const float* mask, size_t n, float step_size,
                            float beta1, float beta2, float one_minus_beta1, float one_minus_beta2,
                            float bias2_sqrt, float eps, int zero_grad, int use_log_flux, const float* bias_dev,
                            void* stream) {
  return jd_adam_step_addends(theta, flux_in, flux_out, grad_flux, exp_avg, exp_avg_sq, mask, n, step_size, beta1, beta2,
                              one_minus_beta1, one_minus_beta2, bias2_sqrt, eps, zero_grad, use_log_flux, bias_dev, nullptr,
                              stream);
}

extern "C" int jd_sgd_step(float* theta, const float* flux_in, float* flux_out, float* grad_flux,
                           const float* mask, size_t n, float lr, int zero_grad, int use_log_flux, void* stream) {
  JD_REQUIRE(theta && flux_in && flux_out && grad_flux && n > 0, "jd_sgd_step: null argument or n == 0");
  OptArgs o{};
  o.a = AdamArgs{theta, flux_in, flux_out, grad_flux, nullptr, nullptr, mask, n,
                 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, lr, zero_grad, 1, use_log_flux ? 0 : 1, nullptr};
  return launch_step(OPT_SGD, o, as_stream(stream));
}

extern "C" int jd_optimizer_step_multi(int n_tensors, float* const* theta, const float* const* grad, float* const* exp_avg,
                                       float* const* exp_avg_sq, float* const* max_exp_avg_sq,
                                       float* const* momentum_buffer, const int* sizes, const float* step_size,
                                       const float* bias2_sqrt, const int* first_step, const jd_optimizer_options* options,
                                       const float* bias_dev, void* stream) {
  JD_REQUIRE(theta && grad && sizes, "jd_optimizer_step_multi: null argument");
  JD_REQUIRE(n_tensors >= 1 && n_tensors <= OPT_MULTI_MAX, "jd_optimizer_step_multi: n_tensors = %d not in [1, %d]", n_tensors,
             OPT_MULTI_MAX);
  int kind = 0;
  OptMultiArgs a{};
  if (int status = read_options(options, "jd_optimizer_step_multi", kind, a.t)) return status;
  const bool adam = opt_moments(kind);
  JD_REQUIRE(!adam || (exp_avg && exp_avg_sq && (bias_dev || (step_size && bias2_sqrt))),
             "jd_optimizer_step_multi: Adam needs its moments and bias terms");
  JD_REQUIRE(kind != OPT_AMSGRAD || max_exp_avg_sq, "jd_optimizer_step_multi: amsgrad needs max_exp_avg_sq");
  JD_REQUIRE(kind != OPT_MOMENTUM || (momentum_buffer && first_step), "jd_optimizer_step_multi: momentum needs momentum_buffer and first_step");
  float* const* third = kind == OPT_AMSGRAD ? max_exp_avg_sq : (kind == OPT_MOMENTUM ? momentum_buffer : nullptr);
  for (int i = 0; i < n_tensors; ++i) {
    JD_REQUIRE(theta[i] && grad[i] && sizes[i] > 0 && (!adam || (exp_avg[i] && exp_avg_sq[i])) && (!third || third[i]),
               "jd_optimizer_step_multi: null tensor %d", i);
    a.theta[i] = theta[i], a.grad[i] = grad[i], a.size[i] = sizes[i];
    if (adam) a.m[i] = exp_avg[i], a.v[i] = exp_avg_sq[i];
    if (third) a.s[i] = third[i];
    if (adam && !bias_dev) a.step_size[i] = step_size[i], a.bias2_sqrt[i] = bias2_sqrt[i];
    if (kind == OPT_MOMENTUM && first_step[i]) a.first_step |= 1ull << i;
  }
  if (adam) {
    a.beta1 = options->beta1, a.beta2 = options->beta2, a.one_minus_beta1 = options->one_minus_beta1;
    a.one_minus_beta2 = options->one_minus_beta2, a.eps = options->eps, a.bias_dev = bias_dev;
  } else {
    a.lr = (float)options->lr;
  }
  return launch_step_multi(kind, n_tensors, a, as_stream(stream));
}

extern "C" int jd_adam_step_multi(int n_tensors, float* const* theta, const float* const* grad, float* const* exp_avg,
                                  float* const* exp_avg_sq, const int* sizes, const float* step_size,
                                  const float* bias2_sqrt, float beta1, float beta2, float one_minus_beta1,
                                  float one_minus_beta2, float eps, const float* bias_dev, void* stream) {
  JD_REQUIRE(theta && grad && exp_avg && exp_avg_sq && sizes && (bias_dev || (step_size && bias2_sqrt)),
             "jd_adam_step_multi: null argument");
  JD_REQUIRE(n_tensors >= 1 && n_tensors <= OPT_MULTI_MAX, "jd_adam_step_multi: n_tensors = %d not in [1, %d]", n_tensors,
             OPT_MULTI_MAX);
  OptMultiArgs a{};
  for (int i = 0; i < n_tensors; ++i) {
    JD_REQUIRE(theta[i] && grad[i] && exp_avg[i] && exp_avg_sq[i] && sizes[i] > 0, "jd_adam_step_multi: null tensor %d", i);
    a.theta[i] = theta[i], a.grad[i] = grad[i], a.m[i] = exp_avg[i], a.v[i] = exp_avg_sq[i], a.size[i] = sizes[i];
    if (!bias_dev) a.step_size[i] = step_size[i], a.bias2_sqrt[i] = bias2_sqrt[i];
  }
  a.bias_dev = bias_dev;
  a.beta1 = beta1, a.beta2 = beta2, a.one_minus_beta1 = one_minus_beta1, a.one_minus_beta2 = one_minus_beta2, a.eps = eps;
  return launch_step_multi(OPT_ADAM, n_tensors, a, as_stream(stream));
}
