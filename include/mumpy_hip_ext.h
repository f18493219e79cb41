/* mumpy_hip_ext.h — entry points of libmumpy_hip.so added after the surface of mumpy_hip.h was frozen (MUMPY_ABI_VERSION 2).
 *
 * The conventions are those of mumpy_hip.h: plain C, raw DEVICE pointers + sizes + `void* stream` last, the CALLER allocates and
 * owns every buffer, nothing here allocates or synchronises (every launching call may be captured into a hipGraph; pointer tables
 * are HOST arrays read at call time), 0 on success, a negative MUMPY_E* code for a rejected argument (nothing is launched), a
 * positive hipError_t for a failed launch, the message in mumpy_last_error().  This header has a version of its own.
 */
#ifndef MUMPY_HIP_EXT_H
#define MUMPY_HIP_EXT_H

#include "mumpy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MUMPY_EXT_VERSION 1
int mumpy_ext_version(void);

/* ---- skipping the update of a step whose gradient is non-finite (what torch's GradScaler.step does with an inf) ----
 * One decision per step, taken on the device at the head of the update from the statistics mumpy_grad_norm_finish left:
 *   skip = any stats[s][2] > 0 (a non-finite gradient element) || any isnan(stats[s][0]) (a NaN norm)
 * over the n_stats (1 ... 8) statistics buffers of the step: if ANY group's gradient is non-finite NO group is updated.  A finite
 * gradient whose square overflows (count 0, norm +Inf) is not skipped.
 *
 * mumpy_update_gate: one single-workgroup launch, after every mumpy_grad_norm_finish of the step and before its updates.
 *   stats           HOST table of n_stats DEVICE statistics buffers (4-byte aligned; only words 0 and 2 are read)
 *   gate            DEVICE, 8 x uint32, 4-byte aligned, zero before the first call; every word is written by every call:
 *                     gate[0] = skip (0 / 1)          gate[1] = updates skipped in total     gate[2] = consecutive skips (0 after
 *                     an applied update)              gate[3] = updates seen                 gate[4] = longest run of skips
 *                     gate[5 ... 7] = 0 (reserved)
 *   hyper_dev, optimizer_kind   HOST tables, one entry per group (1 ... 8 groups: every optimizer of the step): the staged DEVICE
 *                   constants of the group's *_step_dev and its MUMPY_OPT_* kind.  hyper_dev[g] is required (and 4-byte aligned)
 *                   for MUMPY_OPT_ADAMW and ignored otherwise.
 *   applied         DEVICE, `groups` x int64, 8-byte aligned: updates APPLIED to group g so far; advanced by one unless skip.
 *   adam_raw        DEVICE, `groups` x 4 doubles, 8-byte aligned: row g = what mumpy_adamw_gate_hyper wrote for this step of an
 *                   AdamW group {lr, beta1, beta2, t = the NOMINAL step count the staged hyper_dev[g] was derived from}; rows of
 *                   other kinds are not read.
 * AdamW's bias corrections follow the applied count t_eff = applied[g] (after this call): where t_eff == t nothing in hyper_dev[g]
 * is touched -- a run that never skips is bitwise the ungated one -- otherwise step_size = fp32(lr / (1 - beta1^t_eff)) and
 * bc2_sqrt = fp32(sqrt(1 - beta2^t_eff)) are recomputed in double and overwrite those two floats; the other six (the gradient scale
 * among them, which belongs to the clip) are never written.  On a skipped step hyper_dev is left alone.
 * Everything is written by one thread with ordinary stores, in a fixed order. */
int mumpy_adamw_gate_hyper(double* out4_host, double lr, double beta1, double beta2, int step);
int mumpy_update_gate(const float* const* stats, int n_stats, uint32_t* gate, float* const* hyper_dev,
                      const int* optimizer_kind, int groups, int64_t* applied, const double* adam_raw, void* stream);

/* mumpy_adamw_step_dev / mumpy_sgd_step_dev / mumpy_rmsprop_step_dev behind the gate: when gate[0] != 0 every workgroup returns
 * before its first load of param (nothing in param, grad or a state buffer is read or written); when gate[0] == 0 the update is
 * the ungated one bit for bit (same kernel body, same grid).  gate: DEVICE, required, 4-byte aligned.  n >= 1.  The other arguments
 * as in mumpy_hip.h (momentum_buf NULL <=> momentum 0). */
int mumpy_adamw_step_gated_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                               const float* hyper_dev, const uint32_t* gate, void* stream);
int mumpy_sgd_step_gated_dev(float* param, const float* grad, float* momentum_buf, int64_t n, const float* hyper_dev,
                             int nesterov, const uint32_t* gate, void* stream);
int mumpy_rmsprop_step_gated_dev(float* param, const float* grad, float* square_avg, float* momentum_buf, int64_t n,
                                 const float* hyper_dev, const uint32_t* gate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUMPY_HIP_EXT_H */
