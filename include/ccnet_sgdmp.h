/* ccnet_sgdmp.h -- C ABI of libccnet_sgdmp.so: the optimiser step of ccnet_sgd.h (momentum SGD with weight decay, dampening 0,
 * no Nesterov, the in-place zero_grad() and the poly learning rate, a whole parameter list in one launch) for a list that mixes
 * float32 parameters with bf16 parameters whose truth is a float32 master copy.
 *
 * The tensor table: CCNET_SGDMP_TENSOR_WORDS int64 per tensor: P, G, B, NUMEL and GROUP as in ccnet_sgd.h, then M, the device
 * address of the tensor's float32 master (0: none).
 *
 * M == 0, a float32 row: p, g and b are float32 and the step is ccnet_sgd_step's, operation by operation; the results are
 * bit-identical to that entry point's on the same inputs.
 *
 * M != 0, a master row: p and g are bf16, m and b float32.  Per element, each float operation rounded on its own (no fused
 * multiply-add):
 *   g32 = float(g)            exact: the bf16 bits in the upper half of a float32
 *   d   = g32 + wd * m        fl(wd * m), then fl(g32 + .)
 *   b'  = mu * b + d          fl(mu * b), then fl(. + d)
 *   m'  = m - lr * b'         fl(lr * b'), then fl(m - .)
 *   p'  = bf16_rne(m')
 *   g'  = +0 when zero_grads, else g (not written)
 * p is never read: the master is the truth.  That is 22 bytes per element (read g 2, m 4, b 4; write m 4, b 4, p 2, g 2).
 * bf16_rne rounds the float32 bit pattern u to nearest, ties to even, in integers: (u + 0x7FFF + ((u >> 16) & 1)) >> 16.  It is
 * exact for every finite value and for infinities; a value past the largest bf16 rounds to infinity; subnormals and the sign of
 * zero are kept; a NaN gives a NaN ((u >> 16) | 0x40).  Non-finite values otherwise propagate as the formulas say.
 *
 * A tensor whose G is 0 is skipped entirely: neither its p nor its m nor its b is read or written.
 *
 * The chunk table, the two copies of both tables, the groups by value, the schedule with its counter and the one-thread advance
 * behind the step, `cap` and the stream are ccnet_sgd.h's; ccnet_sgdmp_plan writes the same table as ccnet_sgd_plan.  One kernel
 * serves both kinds of row; its path is chosen per chunk from the table row, the same for every lane.  A master row whose p, g,
 * m and b are all 16-byte aligned moves eight elements per lane (one 16-byte vector of g and of p, two each of m and b) with the
 * tensor's last numel % 8 elements on their own; any other master row moves element by element.  A float32 row moves as in
 * ccnet_sgd.h.  Nothing synchronises with the host, nothing is allocated and nothing is copied, so the call can be captured into
 * a graph and replayed with the schedule moving on.
 *
 * Limits, checked before anything is launched: those of ccnet_sgd.h, and for a master row m and b 4-byte aligned, p and g 2-byte
 * aligned.  Return codes: 0 ok, -1 tensor count, -2 NULL table, -3 element count, -4 launch failure, -5 chunk table, -6 group,
 * -7 schedule, -8 tensor pointer (ccnet_sgdmp_last_error_string says which).
 */
#ifndef CCNET_SGDMP_H
#define CCNET_SGDMP_H

#include <stddef.h>
#include <stdint.h>

#include "ccnet_sgd.h" /* CCNET_SGD_CHUNK, _MAX_GROUPS, _MAX_TENSORS, _DEFAULT_CAP: one chunk size and one set of limits for both */

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_SGDMP_VERSION 100

/* one tensor's row: int64[CCNET_SGDMP_TENSOR_WORDS] */
#define CCNET_SGDMP_TENSOR_WORDS 6
#define CCNET_SGDMP_P 0               /* device address of the parameter: bf16 in a master row, float32 otherwise */
#define CCNET_SGDMP_G 1               /* device address of its gradient, of the parameter's type; 0: none, the tensor is skipped */
#define CCNET_SGDMP_B 2               /* device address of its float32 momentum buffer */
#define CCNET_SGDMP_NUMEL 3
#define CCNET_SGDMP_GROUP 4
#define CCNET_SGDMP_M 5               /* device address of its float32 master, 0: a float32 row */

int ccnet_sgdmp_version(void);
const char *ccnet_sgdmp_arch(void);
const char *ccnet_sgdmp_last_error_string(void);

/* Host only; ccnet_sgd_plan's arguments and ccnet_sgd_plan's table. */
int ccnet_sgdmp_plan(const int64_t *numel, int n_tensors, int32_t *chunks, int64_t capacity, int64_t *n_chunks);

/* One optimiser step over the table.  lr, wd and mu are host arrays of n_groups floats, read before the call returns. */
int ccnet_sgdmp_step(const int64_t *tensors_host, const int64_t *tensors_device, int n_tensors, const int32_t *chunks_host,
                     const int32_t *chunks_device, int64_t n_chunks, const float *lr, const float *wd, const float *mu,
                     int n_groups, const float *schedule, int schedule_len, int32_t *counter, int zero_grads, int cap,
                     void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_SGDMP_H */
