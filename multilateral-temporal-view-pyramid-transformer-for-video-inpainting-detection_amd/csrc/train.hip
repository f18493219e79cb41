// train.hip — the training tail of config 5: mask loss forward+backward and the fused AdamW update.
//
// mask loss = softIoULoss + WeightedFocalLoss on the (B, P = H*W) logits, as train.py:107-113 calls them:
//   * softIoU (loss.py:27-42) with e = 0: train.py passes `recall` (False) in the `e` slot (loss.py:49), so the 1e-6 guard
//     is gone.  per sample  cost_b = 1 - sum(p t) / sum(p + t - p t),  p = sigmoid(z);  loss_iou = mean_b cost_b.
//   * focal (loss.py:6-24) with alpha = [1,1], gamma = 2:  f = (1 - exp(-bce))^2 * bce,  bce = BCE-with-logits(z, t);
//     loss_focal = mean over all B*P elements.
//   gradient wrt the logits, closed form (what autograd produces on the reference):
//     d iou   / dz_i = -(t_i D - N (1 - t_i)) / D^2 * p_i (1 - p_i) / B
//     d focal / dz_i = (2 (1 - pt) pt bce + (1 - pt)^2) (p_i - t_i) / (B P),   pt = exp(-bce)
// Two passes over the logits (HBM-bound, 8 B + 12 B per element): per-(sample, split) partial sums, then the gradient;
// every reduction runs in a fixed order (no atomics), so loss and gradient are bitwise reproducible.
//
// AdamW: torch.optim.AdamW single-tensor semantics (utils/utils.py:258; decoupled weight decay, bias correction) over a
// FLAT parameter buffer: one launch per parameter group instead of one per tensor.  28 B of HBM traffic per parameter.
// SGD and RMSprop, the other two branches of get_optimizer (utils/utils.py:252-261), the same way: torch.optim.SGD (coupled
// weight decay, momentum, dampening 0, optional Nesterov; 20 B per parameter with momentum, 12 B without) and
// torch.optim.RMSprop (uncentered; 20 B per parameter, 28 B with momentum).
#include <string.h>
#include "common.h"
using namespace mumpy;

namespace {

constexpr int LOSS_THREADS = 256;

struct ElemLoss {
    float p, bce, pt;
};

__device__ __forceinline__ ElemLoss elem_loss(float z, float t) {
    ElemLoss e;
    const float az = fabsf(z);
    const float ez = __expf(-az);                       // exp(-|z|) in (0,1]
    e.p = (z >= 0.f) ? 1.0f / (1.0f + ez) : ez / (1.0f + ez);
    e.bce = fmaxf(z, 0.f) - z * t + log1pf(ez);         // BCE with logits, the stable form torch uses
    e.pt = __expf(-e.bce);
    return e;
}

__device__ __forceinline__ float block_sum(float v, float* red) {     // fixed-order block reduction, result in all threads
    v = wave_sum(v, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LOSS_THREADS / 64; ++w) s += red[w];
    return s;
}

// pass A: partial[b][split] = {sum p t, sum (p + t - p t), sum focal}
__global__ __launch_bounds__(LOSS_THREADS) void mask_loss_partial_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                         float* __restrict__ partial, int64_t P, int nsplit) {
    __shared__ float red[LOSS_THREADS / 64];
    const int b = blockIdx.y, sp = blockIdx.x;
    const int64_t chunk = (P + nsplit - 1) / nsplit;
    const int64_t beg = sp * chunk, end = (beg + chunk < P) ? beg + chunk : P;
    const float* zb = z + (int64_t)b * P;
    const float* tb = t + (int64_t)b * P;
    float n = 0.f, d = 0.f, f = 0.f;
    for (int64_t i = beg + threadIdx.x; i < end; i += LOSS_THREADS) {
        const float tv = tb[i];
        const ElemLoss e = elem_loss(zb[i], tv);
        n += e.p * tv;
        d += e.p + tv - e.p * tv;
        const float om = 1.0f - e.pt;
        f += om * om * e.bce;
    }
    n = block_sum(n, red);
    d = block_sum(d, red);
    f = block_sum(f, red);
    if (threadIdx.x == 0) {
        float* o = partial + ((int64_t)b * nsplit + sp) * 3;
        o[0] = n; o[1] = d; o[2] = f;
    }
}

// pass B: loss3 = {total, iou, focal} (block (0,0)) and dlogits
__global__ __launch_bounds__(LOSS_THREADS) void mask_loss_grad_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                      const float* __restrict__ partial, float* __restrict__ dz,
                                                                      float* __restrict__ loss3, int B, int64_t P, int nsplit,
                                                                      float eps, float scale) {
    __shared__ float nd[2];
    const int b = blockIdx.y, sp = blockIdx.x;
    if (threadIdx.x == 0) {
        float n = 0.f, d = 0.f;
        for (int s = 0; s < nsplit; ++s) {
            n += partial[((int64_t)b * nsplit + s) * 3 + 0];
            d += partial[((int64_t)b * nsplit + s) * 3 + 1];
        }
        nd[0] = n; nd[1] = d + eps;
        if (b == 0 && sp == 0) {                                         // the scalar losses, samples in order
            float iou = 0.f, foc = 0.f;
            for (int bb = 0; bb < B; ++bb) {
                float nn = 0.f, dd = 0.f;
                for (int s = 0; s < nsplit; ++s) {
                    const float* q = partial + ((int64_t)bb * nsplit + s) * 3;
                    nn += q[0]; dd += q[1]; foc += q[2];
                }
                iou += 1.0f - nn / (dd + eps);
            }
            iou /= (float)B;
            foc /= (float)B * (float)P;
            loss3[0] = (iou + foc) * scale; loss3[1] = iou; loss3[2] = foc;
        }
    }
    __syncthreads();
    if (!dz) return;
    const float N = nd[0], D = nd[1];
    const float inv_d2 = 1.0f / (D * D);
    const float wi = scale / (float)B, wf = scale / ((float)B * (float)P);
    const int64_t chunk = (P + nsplit - 1) / nsplit;
    const int64_t beg = sp * chunk, end = (beg + chunk < P) ? beg + chunk : P;
    const float* zb = z + (int64_t)b * P;
    const float* tb = t + (int64_t)b * P;
    float* db = dz + (int64_t)b * P;
    for (int64_t i = beg + threadIdx.x; i < end; i += LOSS_THREADS) {
        const float tv = tb[i];
        const ElemLoss e = elem_loss(zb[i], tv);
        const float g_iou = -(tv * D - N * (1.0f - tv)) * inv_d2 * e.p * (1.0f - e.p);
        const float om = 1.0f - e.pt;
        const float g_foc = (2.0f * om * e.pt * e.bce + om * om) * (e.p - tv);
        db[i] = wi * g_iou + wf * g_foc;
    }
}

struct AdamHyper {
    float decay, omb1, beta2, omb2, eps, step_size, bc2_sqrt, grad_scale;   // all derived on the host in double
};
struct AdamArgs {
    float* p; const float* g; float* m; float* v;
    int64_t n;
    AdamHyper h;
    const AdamHyper* hdev;      // if set, the hyper-parameters are read from this DEVICE buffer (hipGraph replay: the launch is
                                // frozen at capture, the step-dependent constants are not)
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamHyper& a) {
    g *= a.grad_scale;
    p *= a.decay;                                       // param.mul_(1 - lr * weight_decay)
    m = m + a.omb1 * (g - m);                           // exp_avg.lerp_(grad, 1 - beta1)
    v = a.beta2 * v + a.omb2 * g * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;          // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p -= a.step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
    const AdamHyper hy = a.hdev ? *a.hdev : a.h;
    const int64_t n4 = a.n >> 2;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i], m = reinterpret_cast<f32x4*>(a.m)[i], v = reinterpret_cast<f32x4*>(a.v)[i];
        const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_one(pe, g[e], me, ve, hy);
            p[e] = pe; m[e] = me; v[e] = ve;
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p; reinterpret_cast<f32x4*>(a.m)[i] = m; reinterpret_cast<f32x4*>(a.v)[i] = v;
    }
    const int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x;       // tail (< 4 elements)
    if (i < a.n) adam_one(a.p[i], a.g[i], a.m[i], a.v[i], hy);
}

struct SgdHyper {
    float grad_scale, weight_decay, momentum, lr;       // each rounded from a double once, as the Python floats torch uses
};
struct SgdArgs {
    float* p; const float* g; float* buf;               // buf == nullptr: momentum 0, no buffer
    int64_t n;
    SgdHyper h;
    const SgdHyper* hdev;                               // as AdamArgs::hdev
    int nesterov;
};

// torch.optim.SGD, _single_tensor_sgd with dampening 0, one operation at a time and rounded as torch's kernels round
// (`a.add(b, alpha=c)` is one fma(b, c, a); `mul_` rounds on its own), so a cancelling d = g + wd * p comes out identical:
//   d = grad + wd * p;  buf = buf * momentum + d;  d = nesterov ? d + momentum * buf : buf;  p += -lr * d
template <bool MOM>
__device__ __forceinline__ void sgd_one(float& p, float g, float& b, const SgdHyper& a, bool nesterov) {
#pragma clang fp contract(off)
    float d = fmaf(p, a.weight_decay, g * a.grad_scale);   // grad.add(param, alpha=weight_decay)
    if (MOM) {
        b = b * a.momentum + d;                         // buf.mul_(momentum).add_(d_p, alpha=1 - dampening)
        d = nesterov ? fmaf(b, a.momentum, d) : b;      // d_p.add(buf, alpha=momentum) | buf
    }
    p = fmaf(d, -a.lr, p);                              // param.add_(d_p, alpha=-lr)
}

template <bool MOM>
__global__ __launch_bounds__(256) void sgd_kernel(SgdArgs a) {
    const SgdHyper hy = a.hdev ? *a.hdev : a.h;
    const bool nest = a.nesterov != 0;
    const int64_t n4 = a.n >> 2;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i], b{};
        const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
        if (MOM) b = reinterpret_cast<f32x4*>(a.buf)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = p[e], be = b[e];
            sgd_one<MOM>(pe, g[e], be, hy, nest);
            p[e] = pe; b[e] = be;
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p;
        if (MOM) reinterpret_cast<f32x4*>(a.buf)[i] = b;
    }
    const int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x;       // tail (< 4 elements)
    if (i < a.n) {
        float be = MOM ? a.buf[i] : 0.f;
        sgd_one<MOM>(a.p[i], a.g[i], be, hy, nest);
        if (MOM) a.buf[i] = be;
    }
}

struct RmsHyper {
    float grad_scale, weight_decay, alpha, oma, eps, momentum, lr, pad;   // oma = 1 - alpha (rounded from the double)
};
struct RmsArgs {
    float* p; const float* g; float* sq; float* buf;    // buf == nullptr: momentum 0
    int64_t n;
    RmsHyper h;
    const RmsHyper* hdev;
};

// torch.optim.RMSprop, _single_tensor_rmsprop with centered=False, rounded op by op as torch's kernels round (as sgd_one;
// `addcmul_` is fma(value * t1, t2, self), `addcdiv_` is self + (value * t1) / t2 without fma).  d / den is scale-free, so where d = g + wd * p cancels, one ulp of d moves
// the update by O(1): the rounding of every step has to be torch's, not merely as accurate.
//   d = grad + wd * p;  sq = sq * alpha + (1 - alpha) * d^2;  den = sqrt(sq) + eps;
//   momentum > 0: buf = buf * momentum + d / den, p += -lr * buf;  else p += -lr * (d / den)
template <bool MOM>
__device__ __forceinline__ void rms_one(float& p, float g, float& sq, float& b, const RmsHyper& a) {
#pragma clang fp contract(off)
    const float d = fmaf(p, a.weight_decay, g * a.grad_scale);   // grad.add(param, alpha=weight_decay)
    sq = fmaf(a.oma * d, d, sq * a.alpha);                      // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    const float den = sqrtf(sq) + a.eps;                        // square_avg.sqrt().add_(eps)
    if (MOM) {
        b = b * a.momentum + d / den;                           // buf.mul_(momentum).addcdiv_(grad, avg)
        p = fmaf(b, -a.lr, p);                                  // param.add_(buf, alpha=-lr)
    } else {
        p = p + ((-a.lr) * d) / den;                            // param.addcdiv_(grad, avg, value=-lr): self + value * t1 / t2
    }
}

template <bool MOM>
__global__ __launch_bounds__(256) void rmsprop_kernel(RmsArgs a) {
    const RmsHyper hy = a.hdev ? *a.hdev : a.h;
    const int64_t n4 = a.n >> 2;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i], sq = reinterpret_cast<f32x4*>(a.sq)[i], b{};
        const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
        if (MOM) b = reinterpret_cast<f32x4*>(a.buf)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = p[e], se = sq[e], be = b[e];
            rms_one<MOM>(pe, g[e], se, be, hy);
            p[e] = pe; sq[e] = se; b[e] = be;
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p; reinterpret_cast<f32x4*>(a.sq)[i] = sq;
        if (MOM) reinterpret_cast<f32x4*>(a.buf)[i] = b;
    }
    const int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x;       // tail (< 4 elements)
    if (i < a.n) {
        float be = MOM ? a.buf[i] : 0.f;
        rms_one<MOM>(a.p[i], a.g[i], a.sq[i], be, hy);
        if (MOM) a.buf[i] = be;
    }
}

int64_t update_grid(int64_t n) {               // grid-stride launch of the flat-buffer updates
    int64_t grid = ((n >> 2) + 255) / 256;
    if (grid > 4096) grid = 4096;
    return grid < 1 ? 1 : grid;
}

int loss_splits(int B, int64_t P) {            // enough blocks to fill the chip, chunks of >= 2048 elements
    int64_t s = (1024 + B - 1) / B;
    const int64_t cap = (P + 2047) / 2048;
    if (s > cap) s = cap;
    if (s > 64) s = 64;
    return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" int64_t mumpy_mask_loss_workspace_bytes(int B, int64_t P) {
    if (B <= 0 || P <= 0) return 0;
    return (int64_t)B * loss_splits(B, P) * 3 * (int64_t)sizeof(float);
}

extern "C" int mumpy_mask_loss_fwd_bwd(const float* logits, const float* target, float* dlogits, float* loss3,
                                       void* workspace, int64_t workspace_bytes, int B, int64_t P, float eps,
                                       float loss_scale, void* stream) {
    MUMPY_REQUIRE(logits && target && loss3 && workspace, MUMPY_ENULL, "mask_loss: null pointer");
    MUMPY_REQUIRE(B > 0 && B <= 65535 && P > 0, MUMPY_EINVAL, "mask_loss: bad shape B=%d P=%lld", B, (long long)P);
    MUMPY_REQUIRE(workspace_bytes >= mumpy_mask_loss_workspace_bytes(B, P), MUMPY_EINVAL,
                  "mask_loss: workspace of %lld bytes is too small", (long long)workspace_bytes);
    const int ns = loss_splits(B, P);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(mask_loss_partial_kernel, dim3(ns, B), dim3(LOSS_THREADS), 0, as_stream(stream), logits, target,
                       partial, P, ns);
    MUMPY_CHECK_LAUNCH("mask_loss(partial)");
    hipLaunchKernelGGL(mask_loss_grad_kernel, dim3(ns, B), dim3(LOSS_THREADS), 0, as_stream(stream), logits, target, partial,
                       dlogits, loss3, B, P, ns, eps, loss_scale);
    MUMPY_CHECK_LAUNCH("mask_loss(grad)");
    return 0;
}

static void adam_hyper(AdamHyper& h, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                       double grad_scale) {
    // the scalars torch hands to its fp32 tensor ops are Python doubles rounded once to float: do the same
    h.decay = (float)(1.0 - lr * weight_decay); h.omb1 = (float)(1.0 - beta1); h.beta2 = (float)beta2;
    h.omb2 = (float)(1.0 - beta2); h.eps = (float)eps; h.grad_scale = (float)grad_scale;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    h.step_size = (float)(lr / bc1);
    h.bc2_sqrt = (float)sqrt(bc2);
}

static int adamw_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const AdamHyper* host,
                        const float* hyper_dev, void* stream) {
    MUMPY_REQUIRE(param && grad && exp_avg && exp_avg_sq, MUMPY_ENULL, "adamw: null pointer");
    MUMPY_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq), MUMPY_EALIGN,
                  "adamw: buffers must be 16-byte aligned");
    AdamArgs a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
    a.hdev = reinterpret_cast<const AdamHyper*>(hyper_dev);
    if (host) a.h = *host; else a.h = AdamHyper{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 1.f, 0.f};
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)update_grid(n)), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("adamw");
    return 0;
}

extern "C" int mumpy_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                                double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale,
                                void* stream) {
    if (n == 0) return 0;
    MUMPY_REQUIRE(n > 0 && step >= 1 && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., MUMPY_EINVAL,
                  "adamw: bad arguments (n=%lld step=%d)", (long long)n, step);
    AdamHyper h;
    adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    return adamw_launch(param, grad, exp_avg, exp_avg_sq, n, &h, nullptr, stream);
}

extern "C" int mumpy_adamw_hyper(float* out8, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                                 double grad_scale) {
    MUMPY_REQUIRE(out8, MUMPY_ENULL, "adamw_hyper: null pointer");
    MUMPY_REQUIRE(step >= 1 && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., MUMPY_EINVAL, "adamw_hyper: bad arguments");
    AdamHyper h;
    adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    memcpy(out8, &h, sizeof(h));
    return 0;
}

extern "C" int mumpy_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    const float* hyper_dev, void* stream) {
    if (n == 0) return 0;
    MUMPY_REQUIRE(n > 0 && hyper_dev, MUMPY_EINVAL, "adamw_step_dev: bad arguments");
    return adamw_launch(param, grad, exp_avg, exp_avg_sq, n, nullptr, hyper_dev, stream);
}

// ---- SGD ----
static int sgd_hyper(SgdHyper& h, double lr, double momentum, double dampening, double weight_decay, int nesterov,
                     double grad_scale) {
    MUMPY_REQUIRE(lr >= 0. && momentum >= 0. && weight_decay >= 0., MUMPY_EINVAL, "sgd: bad arguments (lr=%g momentum=%g wd=%g)",
                  lr, momentum, weight_decay);
    MUMPY_REQUIRE(dampening == 0., MUMPY_EINVAL, "sgd: dampening %g is not supported (only 0)", dampening);
    MUMPY_REQUIRE(!nesterov || momentum > 0., MUMPY_EINVAL, "sgd: Nesterov momentum requires a momentum");
    h.grad_scale = (float)grad_scale; h.weight_decay = (float)weight_decay; h.momentum = (float)momentum; h.lr = (float)lr;
    return 0;
}

static int sgd_launch(float* param, const float* grad, float* momentum_buf, int64_t n, const SgdHyper* host,
                      const float* hyper_dev, int nesterov, void* stream) {
    MUMPY_REQUIRE(param && grad, MUMPY_ENULL, "sgd: null pointer");
    MUMPY_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(momentum_buf), MUMPY_EALIGN, "sgd: buffers must be 16-byte aligned");
    MUMPY_REQUIRE(!nesterov || momentum_buf, MUMPY_EINVAL, "sgd: Nesterov momentum requires a momentum buffer");
    SgdArgs a;
    a.p = param; a.g = grad; a.buf = momentum_buf; a.n = n; a.nesterov = nesterov;
    a.hdev = reinterpret_cast<const SgdHyper*>(hyper_dev);
    a.h = host ? *host : SgdHyper{0.f, 0.f, 0.f, 0.f};
    if (momentum_buf)
        hipLaunchKernelGGL(sgd_kernel<true>, dim3((unsigned)update_grid(n)), dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(sgd_kernel<false>, dim3((unsigned)update_grid(n)), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("sgd");
    return 0;
}

extern "C" int mumpy_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, double lr, double momentum,
                              double dampening, double weight_decay, int nesterov, double grad_scale, void* stream) {
    MUMPY_REQUIRE(n >= 0, MUMPY_EINVAL, "sgd: bad size n=%lld", (long long)n);
    SgdHyper h;
    if (int rc = sgd_hyper(h, lr, momentum, dampening, weight_decay, nesterov, grad_scale)) return rc;
    MUMPY_REQUIRE(momentum == 0. || momentum_buf, MUMPY_ENULL, "sgd: momentum %g needs a momentum buffer", momentum);
    if (n == 0) return 0;
    return sgd_launch(param, grad, momentum != 0. ? momentum_buf : nullptr, n, &h, nullptr, nesterov, stream);
}

extern "C" int mumpy_sgd_hyper(float* out4_host, double lr, double momentum, double dampening, double weight_decay,
                               int nesterov, double grad_scale) {
    MUMPY_REQUIRE(out4_host, MUMPY_ENULL, "sgd_hyper: null pointer");
    SgdHyper h;
    if (int rc = sgd_hyper(h, lr, momentum, dampening, weight_decay, nesterov, grad_scale)) return rc;
    memcpy(out4_host, &h, sizeof(h));
    return 0;
}

extern "C" int mumpy_sgd_step_dev(float* param, const float* grad, float* momentum_buf, int64_t n, const float* hyper_dev,
                                  int nesterov, void* stream) {
    MUMPY_REQUIRE(n >= 0 && hyper_dev, MUMPY_EINVAL, "sgd_step_dev: bad arguments");
    if (n == 0) return 0;
    return sgd_launch(param, grad, momentum_buf, n, nullptr, hyper_dev, nesterov, stream);
}

// ---- RMSprop ----
static int rmsprop_hyper(RmsHyper& h, double lr, double alpha, double eps, double weight_decay, double momentum,
                         double grad_scale) {
    MUMPY_REQUIRE(lr >= 0. && alpha >= 0. && eps >= 0. && weight_decay >= 0. && momentum >= 0., MUMPY_EINVAL,
                  "rmsprop: bad arguments (lr=%g alpha=%g eps=%g wd=%g momentum=%g)", lr, alpha, eps, weight_decay, momentum);
    h.grad_scale = (float)grad_scale; h.weight_decay = (float)weight_decay; h.alpha = (float)alpha; h.oma = (float)(1.0 - alpha);
    h.eps = (float)eps; h.momentum = (float)momentum; h.lr = (float)lr; h.pad = 0.f;
    return 0;
}

static int rmsprop_launch(float* param, const float* grad, float* square_avg, float* momentum_buf, int64_t n,
                          const RmsHyper* host, const float* hyper_dev, void* stream) {
    MUMPY_REQUIRE(param && grad && square_avg, MUMPY_ENULL, "rmsprop: null pointer");
    MUMPY_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(square_avg) && aligned16(momentum_buf), MUMPY_EALIGN,
                  "rmsprop: buffers must be 16-byte aligned");
    RmsArgs a;
    a.p = param; a.g = grad; a.sq = square_avg; a.buf = momentum_buf; a.n = n;
    a.hdev = reinterpret_cast<const RmsHyper*>(hyper_dev);
    a.h = host ? *host : RmsHyper{0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    if (momentum_buf)
        hipLaunchKernelGGL(rmsprop_kernel<true>, dim3((unsigned)update_grid(n)), dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(rmsprop_kernel<false>, dim3((unsigned)update_grid(n)), dim3(256), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("rmsprop");
    return 0;
}

extern "C" int mumpy_rmsprop_step(float* param, const float* grad, float* square_avg, float* momentum_buf, int64_t n, double lr,
                                  double alpha, double eps, double weight_decay, double momentum, double grad_scale, void* stream) {
    MUMPY_REQUIRE(n >= 0, MUMPY_EINVAL, "rmsprop: bad size n=%lld", (long long)n);
    RmsHyper h;
    if (int rc = rmsprop_hyper(h, lr, alpha, eps, weight_decay, momentum, grad_scale)) return rc;
    MUMPY_REQUIRE(momentum == 0. || momentum_buf, MUMPY_ENULL, "rmsprop: momentum %g needs a momentum buffer", momentum);
    if (n == 0) return 0;
    return rmsprop_launch(param, grad, square_avg, momentum != 0. ? momentum_buf : nullptr, n, &h, nullptr, stream);
}

extern "C" int mumpy_rmsprop_hyper(float* out8_host, double lr, double alpha, double eps, double weight_decay, double momentum,
                                   double grad_scale) {
    MUMPY_REQUIRE(out8_host, MUMPY_ENULL, "rmsprop_hyper: null pointer");
    RmsHyper h;
    if (int rc = rmsprop_hyper(h, lr, alpha, eps, weight_decay, momentum, grad_scale)) return rc;
    memcpy(out8_host, &h, sizeof(h));
    return 0;
}

extern "C" int mumpy_rmsprop_step_dev(float* param, const float* grad, float* square_avg, float* momentum_buf, int64_t n,
                                      const float* hyper_dev, void* stream) {
    MUMPY_REQUIRE(n >= 0 && hyper_dev, MUMPY_EINVAL, "rmsprop_step_dev: bad arguments");
    if (n == 0) return 0;
    return rmsprop_launch(param, grad, square_avg, momentum_buf, n, nullptr, hyper_dev, stream);
}
