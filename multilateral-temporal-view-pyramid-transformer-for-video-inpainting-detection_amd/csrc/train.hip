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
#include "../../include/mumpy_hip_ext.h"
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
    const unsigned* gate;       // if set and *gate != 0, the update is skipped (mumpy_update_gate): no load of p, g, m or v
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
    if (a.gate && *a.gate) return;                     // one uniform load; the whole grid takes the same branch
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
    const unsigned* gate;                               // as AdamArgs::gate
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
    if (a.gate && *a.gate) return;                     // one uniform load; the whole grid takes the same branch
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
    const unsigned* gate;
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
    if (a.gate && *a.gate) return;                     // one uniform load; the whole grid takes the same branch
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
                        const float* hyper_dev, void* stream, const uint32_t* gate = nullptr) {
    MUMPY_REQUIRE(param && grad && exp_avg && exp_avg_sq, MUMPY_ENULL, "adamw: null pointer");
    MUMPY_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq), MUMPY_EALIGN,
                  "adamw: buffers must be 16-byte aligned");
    AdamArgs a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n; a.gate = gate;
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
                      const float* hyper_dev, int nesterov, void* stream, const uint32_t* gate = nullptr) {
    MUMPY_REQUIRE(param && grad, MUMPY_ENULL, "sgd: null pointer");
    MUMPY_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(momentum_buf), MUMPY_EALIGN, "sgd: buffers must be 16-byte aligned");
    MUMPY_REQUIRE(!nesterov || momentum_buf, MUMPY_EINVAL, "sgd: Nesterov momentum requires a momentum buffer");
    SgdArgs a;
    a.p = param; a.g = grad; a.buf = momentum_buf; a.n = n; a.nesterov = nesterov; a.gate = gate;
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
                          const RmsHyper* host, const float* hyper_dev, void* stream, const uint32_t* gate = nullptr) {
    MUMPY_REQUIRE(param && grad && square_avg, MUMPY_ENULL, "rmsprop: null pointer");
    MUMPY_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(square_avg) && aligned16(momentum_buf), MUMPY_EALIGN,
                  "rmsprop: buffers must be 16-byte aligned");
    RmsArgs a;
    a.p = param; a.g = grad; a.sq = square_avg; a.buf = momentum_buf; a.n = n; a.gate = gate;
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

// ---- gradient-norm clipping on the flat buffers (torch.nn.utils.clip_grad_norm_, L2) ----
// Two kinds of launch, both replayable in a captured step.  The partial kernel streams one group's flat gradient once (4 B per
// parameter) and leaves one fp32 sum of squares and one count of non-finite elements per workgroup.  The finish kernel (one
// workgroup) adds the partials of up to 8 groups in double, reads each group's incoming gradient scale s_g from the scale slot of its
// hyper_dev buffer, forms total = sqrt(sum_g s_g^2 sumsq_g) and coef = min(1, max_norm / (total + 1e-6)) as torch does, and
// multiplies the scale slots by coef: the update kernels then consume the clipped gradient without a second pass over it and without
// a host round trip.  The gradient buffers themselves are never written.
// Every sum runs in a fixed order and the grid is a pure function of n (never of the CU count): the result is bitwise the same on
// every launch and on every device.  Squares are not rescaled: a gradient whose square overflows fp32 gives an infinite norm, as
// torch's fp32 norm does.
namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_UNROLL = 4;                   // independent 16-B loads (and vector accumulators) per thread and sweep
constexpr int GN_SWEEP = GN_THREADS * GN_UNROLL * 4;      // elements one workgroup reads per sweep (16 KB)
constexpr int GN_MAX_PARTIALS = 2048;          // 8 workgroups per CU on 256 CUs; 8 groups x 2048 partials is still one workgroup's finish
constexpr int GN_MAX_GROUPS = 8;

int grad_norm_grid(int64_t n) {
    int64_t grid = (n + GN_SWEEP - 1) / GN_SWEEP;
    if (grid > GN_MAX_PARTIALS) grid = GN_MAX_PARTIALS;
    return grid < 1 ? 1 : (int)grid;
}

__device__ __forceinline__ unsigned non_finite(float v) {            // Inf or NaN: exponent all ones
    return (__builtin_bit_cast(unsigned, v) & 0x7fffffffu) > 0x7f7fffffu ? 1u : 0u;
}

// partial[b] = sum of squares over workgroup b's share, bad[b] = its non-finite elements.  A thread's 16 scalar accumulators take one
// term per sweep each; they are combined pairwise in a fixed order, then the wave's butterfly, then the four waves in order.
__global__ __launch_bounds__(GN_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                                        float* __restrict__ partial, unsigned* __restrict__ bad) {
    __shared__ float red[GN_THREADS / 64];
    __shared__ unsigned redc[GN_THREADS / 64];
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * (GN_THREADS * GN_UNROLL);
    f32x4 acc[GN_UNROLL];
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * (GN_THREADS * GN_UNROLL) + threadIdx.x; i < n4; i += stride) {
        f32x4 v[GN_UNROLL];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) {                        // the loads of a sweep are issued before their use
            const int64_t j = i + u * GN_THREADS;
            v[u] = j < n4 ? g4[j] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) {
            acc[u] += v[u] * v[u];
            cnt += non_finite(v[u][0]) + non_finite(v[u][1]) + non_finite(v[u][2]) + non_finite(v[u][3]);
        }
    }
    const f32x4 q = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    float s = (q[0] + q[1]) + (q[2] + q[3]);
    if (blockIdx.x == 0 && (n4 << 2) + threadIdx.x < n) {            // tail (< 4 elements)
        const float t = g[(n4 << 2) + threadIdx.x];
        s += t * t;
        cnt += non_finite(t);
    }
    s = wave_sum(s, 64);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave] = s; redc[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        bad[blockIdx.x] = (redc[0] + redc[1]) + (redc[2] + redc[3]);
    }
}

struct GradNormFinishArgs {
    const float* partials[GN_MAX_GROUPS];      // per group: np sums of squares, then np counts
    float* hyper[GN_MAX_GROUPS];
    int np[GN_MAX_GROUPS];
    int slot[GN_MAX_GROUPS];                   // index of the gradient-scale float in the group's hyper_dev
    float* stats;
    float max_norm;
    int groups, clip;
};

__global__ __launch_bounds__(GN_THREADS) void grad_norm_finish_kernel(GradNormFinishArgs a) {
    __shared__ double red[GN_THREADS];
    __shared__ unsigned long long redc[GN_THREADS];
    __shared__ float coef_s;
    const int tid = threadIdx.x;
    double total2 = 0.0;                       // thread 0 only
    unsigned long long bad = 0;
    for (int g = 0; g < a.groups; ++g) {
        const float* ps = a.partials[g];
        const unsigned* pc = reinterpret_cast<const unsigned*>(ps) + a.np[g];
        constexpr int PER = GN_MAX_PARTIALS / GN_THREADS;          // a thread's partials: tid, tid + 256, ...; all loaded, then added in order
        float v[PER];
        unsigned k[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = tid + u * GN_THREADS;
            v[u] = i < a.np[g] ? ps[i] : 0.f;
            k[u] = i < a.np[g] ? pc[i] : 0u;
        }
        double s = 0.0;
        unsigned long long c = 0;
#pragma unroll
        for (int u = 0; u < PER; ++u) { s += (double)v[u]; c += k[u]; }
        __syncthreads();
        red[tid] = s; redc[tid] = c;
        __syncthreads();
        for (int o = GN_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) { red[tid] += red[tid + o]; redc[tid] += redc[tid + o]; }
            __syncthreads();
        }
        if (tid == 0) {
            const double sg = (double)a.hyper[g][a.slot[g]];
            a.stats[4 + g] = (float)(fabs(sg) * sqrt(red[0]));
            total2 += sg * sg * red[0];
            bad += redc[0];
        }
    }
    if (tid == 0) {
        const float total = (float)sqrt(total2);
        float coef = 1.0f;
        if (a.clip) {                                                // clip_coef = max_norm / (total_norm + 1e-6), clamped to 1.0
            const float c = __fdiv_rn(a.max_norm, total + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;                              // (a NaN stays a NaN, as under torch.clamp)
        }
        a.stats[0] = total; a.stats[1] = coef;
        a.stats[2] = bad > 16777216ull ? 16777216.0f : (float)bad;   // saturates where fp32 stops counting exactly
        a.stats[3] = 0.f;
        coef_s = coef;
    }
    __syncthreads();
    if (a.clip && tid < a.groups) {
        float* h = a.hyper[tid] + a.slot[tid];
        *h = *h * coef_s;
    }
}

}  // namespace

extern "C" int mumpy_grad_norm_partials(int64_t n) { return n < 1 ? 0 : grad_norm_grid(n); }

extern "C" int mumpy_grad_norm_partial(const float* grad, int64_t n, float* partials, void* stream) {
    MUMPY_REQUIRE(grad && partials, MUMPY_ENULL, "grad_norm_partial: null pointer");
    MUMPY_REQUIRE(n >= 1, MUMPY_EINVAL, "grad_norm_partial: bad size n=%lld", (long long)n);
    MUMPY_REQUIRE(aligned16(grad), MUMPY_EALIGN, "grad_norm_partial: the gradient buffer must be 16-byte aligned");
    MUMPY_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 3u) == 0, MUMPY_EALIGN, "grad_norm_partial: partials must be 4-byte aligned");
    const int np = grad_norm_grid(n);
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)np), dim3(GN_THREADS), 0, as_stream(stream), grad, n, partials,
                       reinterpret_cast<unsigned*>(partials) + np);
    MUMPY_CHECK_LAUNCH("grad_norm_partial");
    return 0;
}

extern "C" int mumpy_grad_norm_finish(const float* const* partials, const int64_t* n, float* const* hyper_dev,
                                      const int* optimizer_kind, int groups, int clip, double max_norm, float* stats,
                                      void* stream) {
    MUMPY_REQUIRE(partials && n && hyper_dev && optimizer_kind && stats, MUMPY_ENULL, "grad_norm_finish: null pointer");
    MUMPY_REQUIRE(groups >= 1, MUMPY_EINVAL, "grad_norm_finish: bad group count %d", groups);
    MUMPY_REQUIRE(groups <= GN_MAX_GROUPS, MUMPY_ERANGE, "grad_norm_finish: %d groups (at most %d)", groups, GN_MAX_GROUPS);
    MUMPY_REQUIRE(!clip || max_norm > 0., MUMPY_EINVAL, "grad_norm_finish: max_norm must be positive, got %g", max_norm);
    MUMPY_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 3u) == 0, MUMPY_EALIGN, "grad_norm_finish: stats must be 4-byte aligned");
    GradNormFinishArgs a;
    memset(&a, 0, sizeof(a));
    for (int g = 0; g < groups; ++g) {
        MUMPY_REQUIRE(partials[g] && hyper_dev[g], MUMPY_ENULL, "grad_norm_finish: null pointer (group %d)", g);
        MUMPY_REQUIRE(((reinterpret_cast<uintptr_t>(partials[g]) | reinterpret_cast<uintptr_t>(hyper_dev[g])) & 3u) == 0, MUMPY_EALIGN,
                      "grad_norm_finish: partials and hyper_dev must be 4-byte aligned (group %d)", g);
        MUMPY_REQUIRE(n[g] >= 1, MUMPY_EINVAL, "grad_norm_finish: bad size n=%lld (group %d)", (long long)n[g], g);
        size_t off = 0;
        switch (optimizer_kind[g]) {
            case MUMPY_OPT_ADAMW: off = offsetof(AdamHyper, grad_scale); break;
            case MUMPY_OPT_SGD: off = offsetof(SgdHyper, grad_scale); break;
            case MUMPY_OPT_RMSPROP: off = offsetof(RmsHyper, grad_scale); break;
            default: MUMPY_REQUIRE(false, MUMPY_EINVAL, "grad_norm_finish: unknown optimizer kind %d (group %d)", optimizer_kind[g], g);
        }
        a.partials[g] = partials[g]; a.hyper[g] = hyper_dev[g]; a.np[g] = grad_norm_grid(n[g]); a.slot[g] = (int)(off / sizeof(float));
    }
    a.stats = stats; a.max_norm = clip ? (float)max_norm : 0.f; a.groups = groups; a.clip = clip ? 1 : 0;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_THREADS), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("grad_norm_finish");
    return 0;
}

// ---- skipping the update of a step whose gradient is non-finite (include/mumpy_hip_ext.h) ----
// One launch of one workgroup at the head of the update, after the grad_norm finishes: it turns their statistics into ONE decision
// for the whole step (gate[0]), keeps the skip counters, advances every group's applied-step count unless the step is skipped, and
// makes AdamW's two bias-correction constants follow that count where it has fallen behind the nominal count the host staged them
// from.  The gated *_step_dev launches (the kernels above with AdamArgs::gate set) return at once when gate[0] != 0.
// Everything here is written by thread 0 with ordinary stores, in a fixed order (as grad_norm_finish_kernel's statistics).
namespace {

constexpr int GATE_MAX = 8;                    // statistics buffers, and groups, per step
constexpr int GATE_WORDS = 8;

struct UpdateGateArgs {
    const float* stats[GATE_MAX];
    AdamHyper* hyper[GATE_MAX];                // the staged constants of the AdamW groups; nullptr for the other kinds
    unsigned* gate;
    long long* applied;
    const double* raw;                         // per group {lr, beta1, beta2, nominal t}
    int n_stats, groups;
};

__global__ __launch_bounds__(64) void update_gate_kernel(UpdateGateArgs a) {
    if (threadIdx.x != 0) return;
    bool skip = false;
    for (int s = 0; s < a.n_stats; ++s) {
        const float norm = a.stats[s][0], bad = a.stats[s][2];
        skip = skip || bad > 0.f || norm != norm;
    }
    const unsigned skipped = a.gate[1] + (skip ? 1u : 0u);
    const unsigned run = skip ? a.gate[2] + 1u : 0u;
    const unsigned seen = a.gate[3] + 1u;
    const unsigned longest = run > a.gate[4] ? run : a.gate[4];
    a.gate[0] = skip ? 1u : 0u; a.gate[1] = skipped; a.gate[2] = run; a.gate[3] = seen; a.gate[4] = longest;
    for (int w = 5; w < GATE_WORDS; ++w) a.gate[w] = 0u;
    if (skip) return;                          // nothing is applied: the counts and the staged constants stay
    for (int g = 0; g < a.groups; ++g) {
        const long long t_eff = a.applied[g] + 1;
        a.applied[g] = t_eff;
        if (!a.hyper[g]) continue;
        const double* r = a.raw + 4 * g;
        if (t_eff == (long long)r[3] || t_eff < 1) continue;      // the host's constants are this step's: leave every bit of them
        const double bc1 = 1.0 - pow(r[1], (double)t_eff), bc2 = 1.0 - pow(r[2], (double)t_eff);     // as adam_hyper()
        a.hyper[g]->step_size = (float)(r[0] / bc1);
        a.hyper[g]->bc2_sqrt = (float)sqrt(bc2);
    }
}

bool aligned_to(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

}  // namespace

extern "C" int mumpy_adamw_gate_hyper(double* out4_host, double lr, double beta1, double beta2, int step) {
    MUMPY_REQUIRE(out4_host, MUMPY_ENULL, "adamw_gate_hyper: null pointer");
    MUMPY_REQUIRE(step >= 1 && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., MUMPY_EINVAL, "adamw_gate_hyper: bad arguments");
    out4_host[0] = lr; out4_host[1] = beta1; out4_host[2] = beta2; out4_host[3] = (double)step;
    return 0;
}

extern "C" int mumpy_update_gate(const float* const* stats, int n_stats, uint32_t* gate, float* const* hyper_dev,
                                 const int* optimizer_kind, int groups, int64_t* applied, const double* adam_raw, void* stream) {
    MUMPY_REQUIRE(stats && gate && hyper_dev && optimizer_kind && applied && adam_raw, MUMPY_ENULL, "update_gate: null pointer");
    MUMPY_REQUIRE(n_stats >= 1 && groups >= 1, MUMPY_EINVAL, "update_gate: bad counts (%d statistics buffers, %d groups)", n_stats, groups);
    MUMPY_REQUIRE(n_stats <= GATE_MAX && groups <= GATE_MAX, MUMPY_ERANGE,
                  "update_gate: %d statistics buffers, %d groups (at most %d of each)", n_stats, groups, GATE_MAX);
    MUMPY_REQUIRE(aligned_to(gate, 4), MUMPY_EALIGN, "update_gate: gate must be 4-byte aligned");
    MUMPY_REQUIRE(aligned_to(applied, 8) && aligned_to(adam_raw, 8), MUMPY_EALIGN, "update_gate: applied and adam_raw must be 8-byte aligned");
    UpdateGateArgs a;
    memset(&a, 0, sizeof(a));
    for (int s = 0; s < n_stats; ++s) {
        MUMPY_REQUIRE(stats[s], MUMPY_ENULL, "update_gate: null pointer (statistics buffer %d)", s);
        MUMPY_REQUIRE(aligned_to(stats[s], 4), MUMPY_EALIGN, "update_gate: statistics buffer %d must be 4-byte aligned", s);
        a.stats[s] = stats[s];
    }
    for (int g = 0; g < groups; ++g) {
        const int k = optimizer_kind[g];
        MUMPY_REQUIRE(k == MUMPY_OPT_ADAMW || k == MUMPY_OPT_SGD || k == MUMPY_OPT_RMSPROP, MUMPY_EINVAL,
                      "update_gate: unknown optimizer kind %d (group %d)", k, g);
        if (k != MUMPY_OPT_ADAMW) continue;
        MUMPY_REQUIRE(hyper_dev[g], MUMPY_ENULL, "update_gate: null pointer (hyper_dev of AdamW group %d)", g);
        MUMPY_REQUIRE(aligned_to(hyper_dev[g], 4), MUMPY_EALIGN, "update_gate: hyper_dev must be 4-byte aligned (group %d)", g);
        a.hyper[g] = reinterpret_cast<AdamHyper*>(hyper_dev[g]);
    }
    a.gate = gate; a.applied = reinterpret_cast<long long*>(applied); a.raw = adam_raw; a.n_stats = n_stats; a.groups = groups;
    hipLaunchKernelGGL(update_gate_kernel, dim3(1), dim3(64), 0, as_stream(stream), a);
    MUMPY_CHECK_LAUNCH("update_gate");
    return 0;
}

#define MUMPY_GATED_ARGS(name)                                                                                        \
    MUMPY_REQUIRE(hyper_dev && gate, MUMPY_ENULL, name ": null pointer");                                             \
    MUMPY_REQUIRE(n >= 1, MUMPY_EINVAL, name ": bad size n=%lld", (long long)n);                                      \
    MUMPY_REQUIRE(aligned_to(gate, 4) && aligned_to(hyper_dev, 4), MUMPY_EALIGN, name ": gate and hyper_dev must be 4-byte aligned")

extern "C" int mumpy_adamw_step_gated_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                          const float* hyper_dev, const uint32_t* gate, void* stream) {
    MUMPY_GATED_ARGS("adamw_step_gated_dev");
    return adamw_launch(param, grad, exp_avg, exp_avg_sq, n, nullptr, hyper_dev, stream, gate);
}

extern "C" int mumpy_sgd_step_gated_dev(float* param, const float* grad, float* momentum_buf, int64_t n, const float* hyper_dev,
                                        int nesterov, const uint32_t* gate, void* stream) {
    MUMPY_GATED_ARGS("sgd_step_gated_dev");
    return sgd_launch(param, grad, momentum_buf, n, nullptr, hyper_dev, nesterov, stream, gate);
}

extern "C" int mumpy_rmsprop_step_gated_dev(float* param, const float* grad, float* square_avg, float* momentum_buf, int64_t n,
                                            const float* hyper_dev, const uint32_t* gate, void* stream) {
    MUMPY_GATED_ARGS("rmsprop_step_gated_dev");
    return rmsprop_launch(param, grad, square_avg, momentum_buf, n, nullptr, hyper_dev, stream, gate);
}
