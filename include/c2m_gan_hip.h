/*
 * c2m_gan_hip.h -- C-ABI of the stage-3 GAN additions of libc2m_hip.so (same library, same conventions as c2m_hip.h: device
 * pointers, launches enqueued on `stream`, a c2m_status returned, nothing synchronises, nothing prints).  The entry points
 * live in a header of their own because they are purely additive: c2m_hip.h and c2m_abi_version() are unchanged.
 *
 * What they replace in the reference (mmsr/models/losses.py:397-398, gradient_penalty_loss):
 *
 *   gradients = gradients.view(gradients.size(0), -1)
 *   gradients_penalty = ((gradients.norm(2, dim=1) - 1)**2).mean()
 *
 * and the backward of that expression.  `grad` is the critic's input gradient, fp32 [N, M] contiguous (M = C*H*W).
 */
#ifndef C2M_GAN_HIP_H
#define C2M_GAN_HIP_H

#include "c2m_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch the forward needs (the per-slice partial sums); 0 for invalid sizes. */
size_t c2m_gp_penalty_workspace_bytes(int N, long long M);

/*
 * norms[n] = ||grad[n, :]||_2 and out[0] = mean_n (norms[n] - 1)^2.  Two launches, no atomics: every sum is added in an order
 * that depends on N and M only, so the same input gives the same bits on every call, whatever its alignment.
 */
int c2m_gp_penalty_forward_f32(c2m_stream_t stream, const float* grad, int N, long long M, float* norms, float* out,
                               void* workspace, size_t workspace_bytes);

/*
 * dgrad[n, i] = gout[0] * (2 / N) * (norms[n] - 1) / norms[n] * grad[n, i], and 0 where norms[n] == 0 (the sub-gradient
 * torch uses for the 2-norm at 0).  gout is a device pointer to the incoming gradient of out[0]; nothing is read back.
 */
int c2m_gp_penalty_backward_f32(c2m_stream_t stream, const float* grad, const float* norms, const float* gout, int N,
                                long long M, float* dgrad);

#ifdef __cplusplus
}
#endif

#endif /* C2M_GAN_HIP_H */
