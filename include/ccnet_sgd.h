/* ccnet_sgd.h -- C ABI of libccnet_sgd.so: the optimiser step of train.py (momentum SGD with weight decay, dampening 0, no
 * Nesterov, the in-place zero_grad() and the poly learning rate) over a whole parameter list in one launch.
 *
 * Per element of every tensor that has a gradient, each float operation rounded on its own (no fused multiply-add):
 *   d  = g + wd * p          fl(wd * p), then fl(g + .)
 *   b' = mu * b + d          fl(mu * b), then fl(. + d)
 *   p' = p - lr * b'         fl(lr * b'), then fl(p - .)
 *   g' = 0 when zero_grads, else g (not written)
 * which is torch.optim.SGD's arithmetic; with b zero-filled before the first step, mu * 0 + d = d is torch's "buffer = clone
 * of d", so there is no first-step branch.  Non-finite values propagate as the formulas say.  A tensor whose g is NULL is
 * skipped entirely: neither its p nor its b is read or written.
 *
 * The tensor table: CCNET_SGD_TENSOR_WORDS int64 per tensor (layout below): the device addresses of p, g (0: no gradient)
 * and b, the element count and the index of the tensor's hyper-parameter group.  The chunk table: every tensor cut into chunks
 * of CCNET_SGD_CHUNK elements (the last one of a tensor is short), one (tensor index, chunk index in the tensor) int32 pair per
 * chunk, tensors in order and chunks in order within a tensor; ccnet_sgd_plan writes it.  Both tables are handed over twice, as
 * a host copy, which the entry point checks, and as a device copy, which the kernel reads; nothing is read back from the device.
 *
 * The launch: 256-thread workgroups, min(n_chunks, cap) of them (cap 0: CCNET_SGD_DEFAULT_CAP), each walking the chunk table
 * with a stride of the grid.  A tensor whose p, g and b are all 16-byte aligned moves as 16-byte vectors with its last
 * numel % 4 elements on their own; any other tensor moves element by element.  The hyper-parameters of up to
 * CCNET_SGD_MAX_GROUPS groups travel by value in the kernel's arguments.  With a schedule the kernel reads step = *counter and
 * takes lr = schedule[min(max(step, 0), schedule_len - 1)], for group k fl(lr * lr[k]) (lr[k] is then the group's multiplier,
 * 1.0 being exact), and a one-thread launch of its own, behind the update on the same stream, adds one to *counter; without a
 * schedule lr[k] is the group's learning rate and counter is not touched.  Everything goes on `stream` (NULL = the default
 * stream); nothing synchronises with the host, nothing is allocated and nothing is copied, so the call can be captured into a
 * graph and replayed with the schedule moving on.
 *
 * Limits, checked before anything is launched: 1 <= n_tensors <= CCNET_SGD_MAX_TENSORS; 1 <= numel <= 2^31 - 1; fewer than
 * 2^31 chunks in all; 1 <= n_groups <= CCNET_SGD_MAX_GROUPS and every group index inside them; p and b not NULL; p, g and b
 * 4-byte aligned; the chunk table equal to ccnet_sgd_plan's; a schedule only with a counter and schedule_len >= 1.
 * Return codes: 0 ok, -1 tensor count, -2 NULL table, -3 element count, -4 launch failure, -5 chunk table, -6 group,
 * -7 schedule, -8 tensor pointer (ccnet_sgd_last_error_string says which).
 */
#ifndef CCNET_SGD_H
#define CCNET_SGD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_SGD_VERSION 100

#ifndef CCNET_SGD_CHUNK               /* (a build may name another size to time it: tools/sgd_time.py --lib) */
#define CCNET_SGD_CHUNK 4096          /* elements per chunk; a multiple of 4 * 256 */
#endif
#define CCNET_SGD_MAX_GROUPS 8
#define CCNET_SGD_MAX_TENSORS 65535
#define CCNET_SGD_DEFAULT_CAP 2048    /* workgroups of one launch when cap = 0 */

/* one tensor's row: int64[CCNET_SGD_TENSOR_WORDS] */
#define CCNET_SGD_TENSOR_WORDS 5
#define CCNET_SGD_P 0                 /* device address of the parameter */
#define CCNET_SGD_G 1                 /* device address of its gradient, 0: none, the tensor is skipped */
#define CCNET_SGD_B 2                 /* device address of its momentum buffer */
#define CCNET_SGD_NUMEL 3
#define CCNET_SGD_GROUP 4

int ccnet_sgd_version(void);
const char *ccnet_sgd_arch(void);
const char *ccnet_sgd_last_error_string(void);

/* Host only.  n_chunks[0] <- the length of the chunk table of tensors with these element counts; when `chunks` is not NULL it
   has room for `capacity` pairs and, if that is enough, receives the table (-5 if not). */
int ccnet_sgd_plan(const int64_t *numel, int n_tensors, int32_t *chunks, int64_t capacity, int64_t *n_chunks);

/* One optimiser step over the table.  lr, wd and mu are host arrays of n_groups floats, read before the call returns. */
int ccnet_sgd_step(const int64_t *tensors_host, const int64_t *tensors_device, int n_tensors, const int32_t *chunks_host,
                   const int32_t *chunks_device, int64_t n_chunks, const float *lr, const float *wd, const float *mu,
                   int n_groups, const float *schedule, int schedule_len, int32_t *counter, int zero_grads, int cap,
                   void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_SGD_H */
