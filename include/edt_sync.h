/*
 * edt_sync.h — C ABI of the MI355X (gfx950) outer-loop sync library `libedt_sync.so`.
 *
 * The reference (BarryFutureman/EvolutionaryDistributedTraining) has no FFI: its hot path is
 * Python/PyTorch-CPU code. Each entry point below replaces one piece of that code; the
 * reference location it replaces is cited on the declaration (paths relative to the reference
 * root). The Python shim `evolutionarydistributedtraining_amd` binds these with ctypes and keeps
 * the reference's call surfaces.
 *
 * Conventions
 *  - Every pointer argument named *device* is HBM memory owned by the caller (PyTorch tensors,
 *    `data_ptr()`); the library never allocates device memory and never synchronises.
 *  - `stream` is a hipStream_t (NULL = the legacy default stream). All work is stream-ordered
 *    and asynchronous; every call is hipGraph-capturable.
 *  - Element counts are uint64_t; buffers are flat, parameters laid out back to back in
 *    `model.parameters()` order (the index order the reference's optimizer state uses).
 *  - Scalars arrive as doubles and are rounded exactly as the reference's torch/numpy code
 *    rounds them (fp32 scalar for `mul_`, tensor-dtype `alpha` for `add(..., alpha=)`).
 *  - Return 0 on success or a negative EDT_ERR_* code; edt_last_error() then holds a
 *    thread-local message.
 */
#ifndef EDT_SYNC_H
#define EDT_SYNC_H

#include <stdint.h>

/* ABI revision. 6 (round 6): edt_slerp_gram / edt_slerp_gram_coef removed (the population's
 * triangle layout is a mode of the needed-sums pass; the sharded population uses
 * edt_slerp_needed_*), edt_slerp_seg_table requires the segment sizes. 5 (round 5): the
 * tensor-list outer step's workspace grew (per-tensor tail-mask
 * offsets; edt_outer_list_workspace_bytes), edt_outer_step_list_tail and
 * edt_slerp_population_layout added, edt_slerp_seg_table refuses in-place outputs that overlap
 * another tensor. 4 (round 4): the tensor-list SLERP reads a device pointer table
 * (edt_slerp_seg_table + the *_table entries), edt_slerp_merge_list_speculative takes the segment
 * sizes (full byte-range overlap check), edt_slerp_blend_segments / _blend_table / _refdot_table
 * added, the on-chip-hold form removed. Workspace sizes come from the *_doubles / *_bytes functions
 * of THIS build: a consumer compiled against another revision must be rebuilt
 * (edt_abi_version() != EDT_ABI_VERSION: refuse to run). */
#define EDT_ABI_VERSION 6

#ifdef __cplusplus
extern "C" {
#endif

/* EDT_ABI_VERSION of the loaded library. */
int edt_abi_version(void);

typedef enum { EDT_F32 = 0, EDT_BF16 = 1 } edt_dtype_t;

enum {
    EDT_OK = 0,
    EDT_ERR_ARG = -1,      /* bad argument (null pointer, unsupported dtype pair, K out of range) */
    EDT_ERR_LAUNCH = -2,   /* kernel launch failed (hipGetLastError) */
};

#define EDT_MAX_WORKERS 64   /* workers consumed by one fused launch */

/* ---- DiLoCo outer step ------------------------------------------------------------------
 * Replaces EDT_LM/diloco.py:238-289 (== EDT_LM/diloco_sim.py:233-299):
 *   acc = 0; for k: acc += (theta_k - theta_g) / K      (worker-major, true division by K)
 *   grad = -acc; torch.optim.SGD(lr, momentum, nesterov).step()  (single-tensor CPU path)
 * fused in one pass over HBM. theta_g and momentum are updated in place.
 * dtype pairs (gdt, wdt): (F32,F32), (F32,BF16) [torch promotion: math in fp32], (BF16,BF16)
 * [every op rounded to bf16 as torch's CPU kernels do]. momentum has dtype gdt and is only
 * touched when momentum_coef != 0; has_momentum = 0 reproduces the first step
 * (`buf = grad.clone()`), 1 the carried buffer (`load_state_dict` carry, diloco.py:258-286).
 * theta_k: host array of K device pointers, 1 <= K <= EDT_MAX_WORKERS. */
int edt_outer_step(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                   void* momentum, int has_momentum, uint64_t n,
                   double lr, double momentum_coef, int nesterov, void* stream);

/* edt_outer_step fused with the broadcast of EDT_LM/diloco.py:302-308 (the new global model saved
 * to every worker dir, from which the next inner loops start): the same step, and in the same pass
 * theta_new rounded to the worker dtype (RNE, torch copy_) is stored into the nbcast device
 * buffers bcast[0..nbcast) (n elements of wdt each; a buffer may be one of the theta_k, which are
 * read before they are overwritten, element by element; none may overlap theta_g).
 * Replaces edt_outer_step + nbcast device copies (each re-reading theta). 0 <= nbcast <= 64;
 * nbcast = 0 is edt_outer_step. */
int edt_outer_step_bcast(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                         void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                         int nesterov, void* const* bcast, int nbcast, void* stream);

/* Bit-exact with the reference on a given host: torch's CPU kernels run add(x, y, alpha) as one
 * FMA on their vectorised path but as round(x + round(alpha * y)) on the scalar tail of every
 * contiguous run (the last numel % Vec::size() elements of each at::parallel_for chunk; Vec::size()
 * = 32 bf16 on AVX-512, 16 on AVX2), which differ in bf16 (EDT_LM/diloco.py:252-289's SGD:
 * grad.add(buf, alpha=mu), param.add_(grad, alpha=-lr)). edt_outer_step / edt_pair_merge_to compute
 * the vectorised form on every element; these variants take the tail elements of the reference's
 * host as a bitmask (device, 1 bit per element of the flat arena, bit i & 7 of byte i >> 3; built
 * from the layout, the host's vector width and its thread count) and round those twice. Ignored
 * for fp32 (torch's fp32 tails are FMAs too). tail_bits NULL = the plain functions. */
int edt_outer_step_tail(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                        void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                        int nesterov, const uint8_t* tail_bits, void* stream);
int edt_pair_merge_tail(const void* b1, const void* b2, const void* m1, const void* m2, int wdt,
                        void* theta_out, int gdt, const void* momentum_in, void* momentum_out,
                        int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                        const uint8_t* tail_bits, void* stream);

/* Pseudo-gradient statistics of the step edt_outer_step would take on these operands, read-only
 * (theta and the workers are not written). Per element i and worker k, in theta's dtype g:
 *   d_k = round_g(f32(theta_k[i]) - f32(theta_g[i]))
 *   m   = the step's mean pseudo-gradient: acc = 0; for k in order: acc = round_g(acc +
 *         round_g(d_k / K))   (true division unless K is a power of two, as the step)
 * chunk_desc (device): nchunks chunks {start, length, segment} in edt_slerp_make_chunks' format
 * (length <= 65,536, never across a segment, every element below n). out (device, 8-byte aligned,
 * edt_delta_stats_doubles(K, nchunks) doubles): first the chunk rows [nchunks][3 K + 2]
 *   S_mm = sum m^2 | S_kk[K] = sum d_k^2 | S_km[K] = sum d_k m | nonfinite_mean | nonfinite[K]
 * then the pass's row scratch. Every sum is fp64 in the canonical chunk-sum order of the SLERP
 * passes (per-lane FMA chains in element order, the descending xor butterfly per tile, the binary
 * tree over the 128 tile sums). An element whose d_k is not finite adds nothing to S_kk[k] and
 * S_km[k] and is counted in nonfinite[k]; one whose m is not finite adds nothing to S_mm or any
 * S_km and is counted in nonfinite_mean. The counts are whole numbers stored as doubles (at most
 * 65,536 per chunk, exact). S_km is formed for K <= 8 and written as 0 above. Operands off a
 * 16-byte boundary take scalar loads; the sums are the same. 1 <= K <= EDT_MAX_WORKERS. */
uint64_t edt_delta_stats_doubles(int K, int64_t nchunks);
int edt_delta_stats(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K, uint64_t n,
                    const uint64_t* chunk_desc, int64_t nchunks, double* out, void* stream);

/* edt_outer_step_tail with a clipped pseudo-gradient: grad = round_g((-acc) * grad_scale), one
 * fp32 multiply rounded to theta's dtype, then the unchanged SGD update. grad_scale must be finite
 * and in [0, 1] (EDT_ERR_ARG otherwise); 1.0f gives edt_outer_step_tail's bits. tail_bits may be
 * NULL. No fused broadcast (edt_broadcast_theta after it) and K <= EDT_MAX_WORKERS only. */
int edt_outer_step_scaled(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                          void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                          int nesterov, const uint8_t* tail_bits, float grad_scale, void* stream);

/* The same step for any population size: K > EDT_MAX_WORKERS runs as consecutive launches of
 * <= 64 workers (the reference's worker order), the running sum carried in `workspace` (n
 * elements of theta's dtype: lossless, the sum is rounded to that dtype after every add).
 * K <= 64: identical to edt_outer_step (workspace unused, may be NULL). */
int edt_outer_step_ws(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                      void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                      int nesterov, void* workspace, void* stream);

/* Tensor-list form of edt_outer_step, for parameters that are T separate device allocations
 * (`list(model.parameters())` of models loaded straight to the GPU, the reference's own objects at
 * EDT_LM/diloco.py:231-246): one launch over all tensors, no packing into a flat buffer.
 *   theta_t[T], momentum_t[T]   host arrays of device pointers (momentum_t unused, may be NULL,
 *                               when momentum == 0)
 *   theta_k[K * T]              worker-major: theta_k[k * T + t] is tensor t of worker k
 *   numel[T]                    element count of each tensor (0 allowed)
 * The per-tensor math is exactly edt_outer_step's. The tensor table (pointers, sizes, chunk
 * offsets) is copied into `workspace` (device memory, 8-byte aligned, at least
 * edt_outer_list_workspace_bytes(T, K)) by a stream-ordered copy, so the workspace must not be
 * reused before the launch has run. 1 <= K <= EDT_MAX_WORKERS. */
uint64_t edt_outer_list_workspace_bytes(int T, int K);
int edt_outer_step_list(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                        void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                        double lr, double momentum, int nesterov, void* workspace,
                        uint64_t workspace_bytes, void* stream);
/* edt_outer_step_list with the reference host's bf16 scalar tails (edt_outer_step_tail's rule, r5;
 * replaces EDT_LM/diloco.py:238-289 run on a master whose torch CPU kernels round bf16 tails
 * separately, over `model.parameters()` lists):
 * tail_bits (device, nullable) holds each tensor's 1-bit-per-element mask from byte
 * tail_byte_offset[t] (host array, T entries), indexed by the element's index inside its tensor.
 * gdt must be EDT_BF16 when tail_bits is given. */
int edt_outer_step_list_tail(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                             void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                             double lr, double momentum, int nesterov, const uint8_t* tail_bits,
                             const uint64_t* tail_byte_offset, void* workspace, uint64_t workspace_bytes,
                             void* stream);
/* edt_outer_step_list_tail with a clipped pseudo-gradient (edt_outer_step_scaled's rule on
 * separate tensors): grad = round_g((-acc) * grad_scale), one fp32 multiply rounded to theta's
 * dtype, then the unchanged SGD update. grad_scale must be finite and in [0, 1] (EDT_ERR_ARG
 * otherwise, nothing written); 1.0f gives edt_outer_step_list(_tail)'s bits. tail_bits and
 * tail_byte_offset may be NULL (no tail emulation); given, gdt must be EDT_BF16. The workspace is
 * edt_outer_step_list's (edt_outer_list_workspace_bytes). */
int edt_outer_step_list_scaled(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                               void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                               double lr, double momentum, int nesterov, const uint8_t* tail_bits,
                               const uint64_t* tail_byte_offset, float grad_scale, void* workspace,
                               uint64_t workspace_bytes, void* stream);

/* edt_outer_step_list fused with Streaming DiLoCo's worker merge, over T runs (a run is one
 * contiguous stretch per operand: a tensor, or a view into an arena). The step is
 * edt_outer_step_list's, bit for bit, on the same runs: theta_k are the delta workers (usually
 * snapshots of a fragment taken some inner steps earlier). In the same pass every merge destination
 *   live[j * T + t], j < nmix   (host array of device pointers, worker dtype, numel[t] elements)
 * moves towards v = round_w(theta_new), the value edt_outer_step_bcast stores, by edt_lerp's rule
 * with t = mix in the worker dtype: c0 = (float)(1.0 - mix), c1 = (float)mix,
 *   live = round_w(round_w(c0 * live) + round_w(c1 * v))
 * i.e. edt_lerp(live, v, wdt, live, wdt, wdt, n, mix). Streaming DiLoCo's alpha is 1 - mix.
 * mix == 1.0 is the overwrite: the destination is not read (NaN / Inf in it do not survive) and v is
 * stored, as edt_outer_step_bcast does. mix must be finite and in (0, 1], 1 <= nmix <=
 * EDT_MAX_WORKERS (nmix may differ from K), else EDT_ERR_ARG.
 * Aliasing: live[j * T + t] may be exactly theta_k[j * T + t] (the worker is read before it is
 * overwritten, element by element, by the same thread); any other overlap of a destination with
 * theta, the momentum, a worker or another destination is EDT_ERR_ARG, nothing launched. When
 * every destination is its worker and nmix == K in {1, 2, 3, 4, 8} the worker values the delta
 * loaded are merged from registers. A run takes the vector body when all its K + 2 + nmix
 * pointers are 16-byte aligned. The workspace (edt_outer_list_mix_workspace_bytes(T, K, nmix)) is
 * edt_outer_step_list's with the destination table behind it. */
uint64_t edt_outer_list_mix_workspace_bytes(int T, int K, int nmix);
int edt_outer_step_list_mix(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                            void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                            double lr, double momentum, int nesterov, void* const* live, int nmix,
                            double mix, void* workspace, uint64_t workspace_bytes, void* stream);

/* Tensor-list form of edt_delta_stats: the statistics of the step edt_outer_step_list would take
 * on T separate tensors, read where they lie (nothing is packed, nothing is written but `out` and
 * `workspace`).
 *   theta_t[T], theta_k[K * T], numel[T]   host arrays as edt_outer_step_list's (worker-major;
 *                               numel[t] == 0 allowed: such a tensor has no chunks and its
 *                               pointers are not read)
 *   chunk_desc (device)         nchunks chunks {start, length, segment}: segment s is tensor s,
 *                               start is RELATIVE to the tensor (edt_slerp_make_chunks over the
 *                               tensors' prefix sums, each start minus its tensor's offset), a
 *                               chunk never crosses a tensor, start + length <= numel[segment]
 *   out (device, 8-byte aligned, edt_delta_stats_doubles(K, nchunks) doubles): the chunk rows
 *                               [nchunks][3 K + 2] in edt_delta_stats' layout, then row scratch
 *   workspace (device, 8-byte aligned, >= edt_delta_stats_list_workspace_bytes(T, K)): receives
 *                               the pointer table by a stream-ordered copy, so it must not be
 *                               reused before the launch has run
 * Numerics: the rows of tensor t's chunks equal, bit for bit, the rows edt_delta_stats gives for
 * that tensor alone as an arena of one segment [0, numel[t]): the same d_k, m, masking and counts,
 * and the canonical chunk-sum order with the tile and lane mapping taken from the element's index
 * INSIDE ITS TENSOR (a tensor's aligned body starts at its element 0: no head, a tail of < 8
 * elements). Against edt_delta_stats over the tensors packed into one arena the per-chunk bits
 * agree only when every numel[t] is a multiple of 8 (else the arena's chunk starts are off 8 and
 * its lanes hold other elements); the totals then differ by fp64 summation order alone.
 * A tensor whose K + 1 pointers are all 16-byte aligned takes vector loads, any other scalar loads
 * in the same lane mapping: the bits do not depend on alignment. S_km is formed for K <= 8.
 * 1 <= K <= EDT_MAX_WORKERS, T >= 0 (T == 0 or nchunks == 0: nothing to do). */
uint64_t edt_delta_stats_list_workspace_bytes(int T, int K);
int edt_delta_stats_list(const void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                         const uint64_t* numel, int T, const uint64_t* chunk_desc, int64_t nchunks, double* out,
                         void* workspace, uint64_t workspace_bytes, void* stream);

/* Partial delta sum for the sharded multi-GPU step (EDT_LM/diloco.py:243-246 restricted to the
 * workers resident on this rank): acc_f32[i] (+)= sum_{k<K_local} round_g((theta_k - theta_g)/K_total).
 * accumulate = 0 starts from zero, 1 continues the running fp32 sum already in acc_f32 (so two
 * launches over workers [0,a) and [a,K) add in the same order as one launch over [0,K)).
 * The cross-rank sum then goes over RCCL. */
int edt_delta_partial(const void* theta_g, int gdt, const void* const* theta_k, int wdt,
                      int K_local, int K_total, uint64_t n, float* acc_f32, int accumulate,
                      void* stream);

/* SGD on a shard from a reduced fp32 pseudo-gradient sum: grad = -round_g(acc_f32), then the
 * torch.optim.SGD single-tensor update of EDT_LM/diloco.py:252-289. */
int edt_sgd_apply(void* theta_g, int gdt, const float* acc_f32, void* momentum, int has_momentum,
                  uint64_t n, double lr, double momentum_coef, int nesterov, void* stream);

/* SGD on a shard from nacc per-rank fp32 partial sums of it (acc_f32[0..nacc), device pointers,
 * n elements each), summed in that order: grad = -round_g(((acc_0 + acc_1) + ...) + acc_{nacc-1}).
 * The sharded step's reduce_ordered schedule (all-to-all of the partials, then this): the
 * cross-rank sum has one fixed order, independent of the collective library's algorithm. */
int edt_sgd_apply_sum(void* theta_g, int gdt, const float* const* acc_f32, int nacc, void* momentum,
                      int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, void* stream);

/* The two sharded SGD entries with a clipped pseudo-gradient (edt_outer_step_scaled's rule):
 * grad = round_g((-a) * grad_scale), a the rounded sum edt_sgd_apply(_sum) negates — one fp32
 * multiply rounded to theta's dtype, then the unchanged SGD update. grad_scale must be finite and in
 * [0, 1] (EDT_ERR_ARG otherwise, nothing written); 1.0f gives the unscaled entry's bits. */
int edt_sgd_apply_sum_scaled(void* theta_g, int gdt, const float* const* acc_f32, int nacc, void* momentum,
                             int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                             float grad_scale, void* stream);
int edt_sgd_apply_scaled(void* theta_g, int gdt, const float* acc_f32, void* momentum, int has_momentum,
                         uint64_t n, double lr, double momentum_coef, int nesterov, float grad_scale, void* stream);

/* Statistics of the mean pseudo-gradient a shard owner is about to apply, read-only: per element
 *   m = round_g(((acc_0 + acc_1) + ...) + acc_{nacc-1})     (fp32 adds in that order)
 * which is the value edt_sgd_apply_sum (nacc partials) or edt_sgd_apply (nacc = 1: the reduced
 * shard) negates into the gradient. chunk_desc (device): nchunks chunks in edt_slerp_make_chunks'
 * format over [0, n), the same for every partial. out (device, 8-byte aligned,
 * edt_partial_sum_stats_doubles(nchunks) doubles): first the chunk rows [nchunks][2]
 *   S_mm = sum m^2 | nonfinite_mean
 * then the pass's row scratch. fp64 sums in the canonical chunk-sum order, with edt_delta_stats'
 * tile, lane and tree mapping; an element whose m is not finite adds nothing to S_mm and is
 * counted. Partials off a 16-byte boundary take scalar loads; the sums are the same.
 * 1 <= nacc <= EDT_MAX_WORKERS, gdt EDT_F32 or EDT_BF16. */
uint64_t edt_partial_sum_stats_doubles(int64_t nchunks);
int edt_partial_sum_stats(const float* const* acc_f32, int nacc, int gdt, uint64_t n, const uint64_t* chunk_desc,
                          int64_t nchunks, double* out, void* stream);

/* ---- the sharded fragment step's piece lists (Streaming DiLoCo across ranks) -----------------
 * Fragment space is a fragment's runs laid back to back; a rank's shard of it cuts runs in the
 * middle, so each phase of the sharded fragment step runs over a list of T PIECES: one contiguous
 * stretch of numel[t] elements of every operand, given by one pointer per operand (a view into an
 * arena, or into a compact fragment-space buffer). The three entries share edt_outer_step_list's
 * conventions: host arrays of device pointers, numel[t] == 0 allowed (such a piece's pointers are
 * not read), a device workspace (8-byte aligned, >= the entry's _workspace_bytes) that receives
 * the table by a stream-ordered copy and must not be reused before the launch has run, one launch
 * whatever T. A piece whose pointers are all 16-byte aligned takes vector accesses, any other
 * scalar ones; every result is element-wise, so the bits depend neither on alignment nor on how
 * the pieces are cut. T >= 0 (T == 0: nothing to do). Additive to ABI 6.
 *
 * edt_delta_partial_list — phase 1, edt_delta_partial over pieces, bit for bit:
 *   acc_t[t][i] = sum_{k < K_local} round_g(round_g(f32(theta_k[k * T + t][i]) - f32(theta_t[t][i])) / K_total)
 * the sum in fp32, local workers in order; true division unless K_total is a power of two. theta_t
 * and theta_k are read, acc_t (fp32) is written. 1 <= K_local <= EDT_MAX_WORKERS, K_total >= 1.
 *
 * edt_sgd_sum_list_to — phase 2 on the owned shard's pieces, edt_sgd_apply_sum's sum and update:
 *   a = round_g(((p_0 + p_1) + ...) + p_{nacc-1}),  p_r = parts[r * T + t]  (fp32, rank order)
 *   grad = -a, then the torch.optim.SGD update with momentum_t[t] (updated in place; the table may
 *   be null when momentum_coef == 0).
 * theta_t is ONLY READ: the new theta (theta's dtype) is stored to out_t[t], as edt_sgd_delta_sum_q
 * leaves theta alone. 1 <= nacc <= EDT_MAX_WORKERS.
 *
 * edt_theta_scatter_mix_list — phase 3 on every rank, over a whole bucket's pieces:
 *   theta_t[t][i] = src_t[t][i]                      (theta's dtype, the bits as they are)
 *   v = round_w(src);  live[j * T + t][i] = round_w(round_w(c0 * live) + round_w(c1 * v)),  j < nmix
 * with c0 = (float)(1.0 - mix), c1 = (float)mix: edt_outer_step_list_mix's merge, i.e.
 * edt_lerp(live, v, wdt, live, wdt, wdt, n, mix). mix == 1.0 stores v without reading the
 * destination. mix must be finite and in (0, 1], 0 <= nmix <= EDT_MAX_WORKERS (0: theta only; live
 * may then be null), else EDT_ERR_ARG. Stores follow the EDT_NT_STORES policy. Aliasing: theta's
 * pieces and the destinations are written, so none of them may overlap src, theta, or another
 * destination: EDT_ERR_ARG, nothing launched. */
uint64_t edt_delta_partial_list_workspace_bytes(int T, int K_local);
int edt_delta_partial_list(const void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K_local,
                           int K_total, float* const* acc_t, const uint64_t* numel, int T, void* workspace,
                           uint64_t workspace_bytes, void* stream);
uint64_t edt_sgd_sum_list_to_workspace_bytes(int T, int nacc);
int edt_sgd_sum_list_to(const void* const* theta_t, int gdt, const float* const* parts, int nacc,
                        void* const* momentum_t, int has_momentum, void* const* out_t, const uint64_t* numel, int T,
                        double lr, double momentum_coef, int nesterov, void* workspace, uint64_t workspace_bytes,
                        void* stream);
uint64_t edt_theta_scatter_mix_list_workspace_bytes(int T, int nmix);
int edt_theta_scatter_mix_list(void* const* theta_t, int gdt, const void* const* src_t, void* const* live, int wdt,
                               int nmix, double mix, const uint64_t* numel, int T, void* workspace,
                               uint64_t workspace_bytes, void* stream);

/* ---- block-quantized partial exchange (the sharded step's opt-in "reduce_q" schedule) --------
 * The reference moves checkpoints over a shared disk (EDT_LM/diloco.py:231-235, 302-308) and has
 * no wire format; reduce_ordered ships each rank's pseudo-gradient partial as fp32. These entries
 * ship it as OCP MX blocks instead. Wire format:
 *   block      32 consecutive elements of the fp32 partial share one E8M0 scale byte (bias 127)
 *   scale      e = floor(log2(amax)) - emax, emax = 8 (E4M3) / 2 (E2M1); byte = clamp(e + 127, 0, 254);
 *              an all-zero block (+-0) stores byte 0
 *   elements   v * 2^-e rounded to nearest-even onto the element grid, saturating at +-448 (E4M3,
 *              OCP encoding, never NaN) / +-6 (E2M1); the sign is kept, -0 included
 *   non-finite a block holding any NaN or +-Inf stores scale byte 255 (elements: code 0); every
 *              element of it dequantizes to NaN, so a diverged worker is never hidden
 *   packing    MXFP8 one byte per element; MXFP4 element 2i in the low nibble, 2i+1 in the high
 *              one. A region of R elements is R*bits/8 payload bytes followed by R/32 scale bytes;
 *              R % 512 == 0, so payload and scales both start 16-byte aligned
 *   D(q)       elem * 2^e, exact in fp32
 * fp32 subnormal inputs are outside the bit-exact contract (finite output within one grid step). */
typedef enum { EDT_MXFP8 = 0, EDT_MXFP4 = 1 } edt_qfmt_t;

/* How the encoder picks an element's grid neighbour. EDT_ROUND_NEAREST is the rule above (every entry
 * without _sr). EDT_ROUND_STOCHASTIC (the *_sr entries below; opt-in) keeps blocks,
 * packing, region layout, the non-finite rule and the decoder, and changes the encoder only:
 *   scale      e = floor(log2(amax)) - emax as above; if amax * 2^-e exceeds the element maximum (448 /
 *              6), e + 1 instead, so no finite element of the block saturates; byte = clamp(e + 127, 0,
 *              254) (at the 254 clamp elements may still saturate: outside the unbiased contract); an
 *              all-zero block stores byte 0
 *   elements   a = |v| * 2^-e (exact), k = max(floor(log2 a), EMIN) (EMIN = -6 / 0), q = 2^(k - MB)
 *              (MB = 3 / 1), t = a / q (exact), lo = floor(t), f16 = floor((t - lo) * 2^16); the
 *              element is (lo + up) * q with up = (r16 < f16), r16 the element's 16 random bits. The
 *              sign is kept, for values that round to zero too. A value on the grid never moves
 *              (f16 = 0); P(up) is within 2^-16 of the exact fraction.
 *   r16        Philox4x32 with EDT_PHILOX_ROUNDS rounds (M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 =
 *              0x9E3779B9, W1 = 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter =
 *              (g & 0xffffffff, g >> 32, step & 0xffffffff, stream_id), g = global element index / 8.
 *              The four output words serve elements 8g .. 8g+7: element 8g + j takes bits
 *              16*(j%2) .. 16*(j%2)+15 of word j/2. The bits depend on seed, step, stream_id and the
 *              global element index only — not on the grid, the bucket boundaries or the dtypes.
 * Stochastic rounding takes no residual: it is unbiased in expectation and carries no state beyond
 * the seed and the step counter. */
typedef enum { EDT_ROUND_NEAREST = 0, EDT_ROUND_STOCHASTIC = 1 } edt_round_t;
#define EDT_PHILOX_ROUNDS 10

/* Bytes of one region of region_elems elements (HOST function; 0 for an unknown fmt or a
 * region_elems that is not a multiple of 512). */
uint64_t edt_q_region_bytes(uint64_t region_elems, int fmt);

/* Phase 1: p = edt_delta_partial's fp32 partial (bit-identical, never written to HBM), quantized
 * into `packed` as n / region_elems regions back to back ([dest rank][payload | scales] for one
 * bucket of the schedule). residual (nullable, n floats): error feedback — p' = p + residual is
 * what is quantized (one fp32 add) and residual = p' - D(q) is stored (one fp32 subtract).
 * EDT_ERR_ARG when n % region_elems != 0, region_elems % 512 != 0, fmt is unknown, K is out of
 * range or an operand is not 16-byte aligned. */
int edt_delta_partial_q(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                        int K_total, uint64_t n, uint64_t region_elems, int fmt, float* residual, void* packed,
                        void* stream);

/* edt_delta_partial_q with EDT_ROUND_STOCHASTIC (no residual). elem_base (a multiple of 8) is the
 * global index of the call's first element: element i of the call draws the bits of global element
 * elem_base + i, so a bucketed schedule (one call per bucket, elem_base = the bucket's start) writes
 * the same bytes as one call over the whole arena. EDT_ERR_ARG as edt_delta_partial_q, and when
 * elem_base % 8 != 0. */
int edt_delta_partial_q_sr(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                           int K_total, uint64_t n, uint64_t region_elems, int fmt, void* packed, uint64_t seed,
                           uint64_t step, uint32_t stream_id, uint64_t elem_base, void* stream);

/* Phase 2: edt_sgd_apply_sum on nacc quantized regions of n elements each (regions[0..nacc),
 * device pointers): grad = -round_g(((D(q_0) + D(q_1)) + ...) + D(q_{nacc-1})) in fp32, that
 * order, then the same SGD update. n % 512 == 0; operands 16-byte aligned. */
int edt_sgd_apply_sum_q(void* theta_g, int gdt, const void* const* regions, int nacc, int fmt, void* momentum,
                        int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, void* stream);

/* ---- the sharded fragment step's quantized phases (Streaming DiLoCo's low-precision outer gradients) ----
 * edt_delta_partial_list / edt_sgd_sum_list_to with the partial crossing the links as MX regions (the
 * wire format above, unchanged) instead of fp32. Both entries work on one FRAGMENT-SPACE RANGE
 * [lo, lo + n) of one fragment (lo % 512 == 0) and take its arena operands through ONE PIECE TABLE:
 * T pieces, sorted and disjoint, each inside the range; piece t covers the fragment-space elements
 * [start[t], start[t] + numel[t]) and gives one device pointer per arena operand, to the piece's first
 * element. numel[t] == 0 is allowed (its pointers are not read), T == 0 too. Elements of the range that
 * no piece covers are the padding beyond the fragment's size: they read as +0 for theta and every
 * worker, and nothing of theirs is stored to an arena or to the momentum. The compact operands
 * (residual, packed, regions, momentum, out) are indexed by the element's offset in the range and must
 * be 16-byte aligned. The table is uploaded into `workspace` (8-byte aligned, >= the entry's
 * _workspace_bytes; may be null when that is 0) by a stream-ordered copy, as the _list entries do; one
 * launch whatever T. A lane takes vector loads where its 8 elements lie inside one piece whose arena
 * addresses for them are 16-byte aligned and gathers element by element otherwise; the results do not
 * depend on which. Additive to ABI 6.
 *
 * edt_delta_partial_q_frag — phase 1: p = edt_delta_partial_list's fp32 partial of the range, bit for
 * bit (local workers in order; true division unless K_total is a power of two; +0 on the padding),
 * never written to HBM, then edt_delta_partial_q's rule: with residual (nullable, n floats) p' = p +
 * residual is quantized and residual = p' - D(q) is stored; `packed` receives n / region_elems
 * regions back to back ([dest rank][payload | scales]). theta_k[k * T + t] is worker k's pointer for
 * piece t: into its live arena, or into a compact fragment-space snapshot (base + start[t]).
 * EDT_ERR_ARG, nothing launched: an unknown fmt, region_elems % 512 != 0, n % region_elems != 0,
 * lo % 512 != 0, K out of range, a null pointer of a non-empty piece, pieces unsorted, overlapping or
 * outside the range, packed null, packed or residual off a 16-byte boundary, a missing workspace.
 *
 * edt_sgd_sum_q_frag_to — phase 2 on the owned shard [lo, lo + n) (n % 512 == 0): the nacc received
 * regions of n elements each are dequantized and summed in rank order and the SGD update applied,
 * exactly as edt_sgd_apply_sum_q does; theta_t is ONLY READ. momentum (theta's dtype, n elements,
 * compact; may be null when momentum_coef == 0) is updated in place where a piece covers the element
 * and left alone on the padding; out (theta's dtype, n elements, compact) receives the new theta, and
 * ZERO on the padding. EDT_ERR_ARG as above, and for nacc out of range, a null region or out, a
 * missing momentum buffer, or a compact buffer off a 16-byte boundary. */
uint64_t edt_delta_partial_q_frag_workspace_bytes(int T, int K_local);
int edt_delta_partial_q_frag(const void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K_local,
                             int K_total, const uint64_t* start, const uint64_t* numel, int T, uint64_t lo, uint64_t n,
                             uint64_t region_elems, int fmt, float* residual, void* packed, void* workspace,
                             uint64_t workspace_bytes, void* stream);
uint64_t edt_sgd_sum_q_frag_to_workspace_bytes(int T);
int edt_sgd_sum_q_frag_to(const void* const* theta_t, int gdt, const uint64_t* start, const uint64_t* numel, int T,
                          uint64_t lo, uint64_t n, const void* const* regions, int nacc, int fmt, void* momentum,
                          int has_momentum, void* out, double lr, double momentum_coef, int nesterov, void* workspace,
                          uint64_t workspace_bytes, void* stream);

/* The quantized gather (reduce_q with gather_format): the all-gather of the new theta is replaced
 * by an all-gather of each owner's quantized update, same wire format, and every rank adds the same
 * dequantized update to its replica.
 *
 * Phase 2' over one owned shard of n elements (n % 512 == 0): edt_sgd_apply_sum_q's sum and SGD
 * update in registers,
 *   a = round_g(((D(p_0) + D(p_1)) + ...) + D(p_{nacc-1})), grad = -a, SGD -> theta' and the momentum
 * (the momentum is stored, bit-identical to edt_sgd_apply_sum_q's), then
 *   u = f32(theta') - f32(theta)            one fp32 subtract
 *   u' = u + residual                       one fp32 add, only with residual (error feedback)
 *   q = Q(u') in fmt_out -> packed_out      one region of n elements, [payload | scales]
 *   residual = u' - D(q)                    one fp32 subtract
 * theta_g is NOT written. residual (nullable, n floats) is the owner's error feedback, sharded like
 * the momentum. fmt_in (the regions') and fmt_out are independent. A non-finite update block
 * stores scale byte 255. EDT_ERR_ARG for an unknown format, nacc outside [1, 64], n % 512 != 0, a
 * bad dtype, a null buffer or an operand that is not 16-byte aligned. */
int edt_sgd_delta_sum_q(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in, void* momentum,
                        int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, float* residual,
                        void* packed_out, int fmt_out, void* stream);

/* edt_sgd_delta_sum_q with the update quantized under EDT_ROUND_STOCHASTIC (no residual): the sum,
 * the SGD update and the momentum bits are edt_sgd_delta_sum_q's; element i of the shard draws the
 * bits of global element elem_base + i (elem_base % 8 == 0: the shard's start in the arena). */
int edt_sgd_delta_sum_q_sr(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                           void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                           void* packed_out, int fmt_out, uint64_t seed, uint64_t step, uint32_t stream_id,
                           uint64_t elem_base, void* stream);

/* ---- the guard on reduce_q: measure, clip, and a phase 1 that can be taken back ----
 * Statistics of the mean pseudo-gradient edt_sgd_apply_sum_q / edt_sgd_delta_sum_q are about to
 * apply, read-only: edt_partial_sum_stats with every partial dequantized from its region,
 *   m = round_g(((D(q_0) + D(q_1)) + ...) + D(q_{nacc-1}))     (fp32 adds in that order)
 * quantization error and residuals included. regions[0..nacc): device pointers to packed regions
 * of n elements each in fmt, 16-byte aligned; n % 512 == 0. chunk_desc (device): nchunks chunks over
 * [0, n) whose starts and lengths are multiples of 8 (edt_slerp_make_chunks over a shard gives
 * such a table), so there is no scalar path. out (device, 8-byte aligned,
 * edt_partial_sum_stats_doubles(nchunks) doubles — the same rows and workspace as the fp32 form):
 * the chunk rows [nchunks][2] = S_mm | nonfinite_mean, then the row scratch. The same canonical
 * chunk-sum order, so S_mm equals edt_partial_sum_stats on the dequantized fp32 arrays bit for
 * bit. A scale-255 block is 32 NaN elements: they add nothing to S_mm and are counted.
 * EDT_ERR_ARG for an unknown fmt or gdt, nacc outside [1, 64], n % 512 != 0, a null or misaligned
 * pointer. */
int edt_partial_sum_stats_q(const void* const* regions, int nacc, int fmt, int gdt, uint64_t n,
                            const uint64_t* chunk_desc, int64_t nchunks, double* out, void* stream);

/* Phase 2 and phase 2' with a clipped pseudo-gradient (edt_sgd_apply_sum_scaled's rule on the
 * dequantized rank-ordered sum): grad = round_g((-a) * grad_scale), one fp32 multiply rounded to
 * theta's dtype, then the unchanged SGD update — and, in phase 2', the unchanged quantization of
 * u = theta' - theta. grad_scale must be finite and in [0, 1] (EDT_ERR_ARG otherwise, nothing
 * written); 1.0f gives the unscaled entry's bits (theta or the packed update, the momentum, the
 * residual). Everything else as the unscaled entries. */
int edt_sgd_apply_sum_q_scaled(void* theta_g, int gdt, const void* const* regions, int nacc, int fmt, void* momentum,
                               int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                               float grad_scale, void* stream);
int edt_sgd_delta_sum_q_scaled(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                               void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                               int nesterov, float* residual, void* packed_out, int fmt_out, float grad_scale,
                               void* stream);
int edt_sgd_delta_sum_q_sr_scaled(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                                  void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                                  int nesterov, void* packed_out, int fmt_out, uint64_t seed, uint64_t step,
                                  uint32_t stream_id, uint64_t elem_base, float grad_scale, void* stream);

/* edt_delta_partial_q with error feedback whose new residual goes to a second buffer (the
 * transactional phase 1: a caller that may refuse the step keeps residual_in and swaps the two
 * buffers only when it commits): p' = p + residual_in is quantized and residual_out = p' - D(q).
 * residual_in is only read. Both are n floats, 16-byte aligned and non-null (without error feedback
 * use edt_delta_partial_q); residual_in == residual_out is edt_delta_partial_q bit for bit, any
 * other overlap is EDT_ERR_ARG. The packed bytes are edt_delta_partial_q's. */
int edt_delta_partial_q_to(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                           int K_total, uint64_t n, uint64_t region_elems, int fmt, const float* residual_in,
                           float* residual_out, void* packed, void* stream);

/* Phase 3 over a bucket of n elements: theta = round_g(f32(theta) + D(q)), one fp32 add then RNE to
 * theta's dtype. `packed` holds n / region_elems regions back to back, each of region_elems
 * elements ([src rank][payload | scales]: the mirror of edt_delta_partial_q's layout). The same call
 * with the same bytes on every rank keeps the replicas bit-identical; a block with scale byte 255
 * makes its 32 elements NaN. EDT_ERR_ARG when n % region_elems != 0, region_elems % 512 != 0, fmt
 * or gdt is unknown, or an operand is null or not 16-byte aligned. */
int edt_apply_delta_q(void* theta_g, int gdt, const void* packed, uint64_t n, uint64_t region_elems, int fmt,
                      void* stream);

/* Phase 3 fused with the broadcast of EDT_LM/diloco.py:302-308 (the new global weights handed to
 * every worker): edt_apply_delta_q's update of theta_g, bit for bit, and in the same pass the value
 * written to theta_g, rounded to the worker dtype (RNE, torch copy_), is stored into the nbcast
 * device buffers bcast[0..nbcast) (n elements of wdt each) — what edt_apply_delta_q followed by
 * nbcast copies (each re-reading theta) leaves. (gdt, wdt) is one of edt_outer_step's dtype pairs;
 * 0 <= nbcast <= 64, nbcast = 0 is edt_apply_delta_q. A NaN element of theta (a scale-255 block) is
 * NaN in every destination; its payload bits are not specified. EDT_ERR_ARG as edt_apply_delta_q,
 * and when a destination is null, not 16-byte aligned, or overlaps theta_g or packed. */
int edt_apply_delta_q_bcast(void* theta_g, int gdt, const void* packed, uint64_t n, uint64_t region_elems, int fmt,
                            void* const* bcast, int wdt, int nbcast, void* stream);

/* The broadcast alone, for the schedules whose new theta arrives through the all-gather: theta_g
 * (n elements of gdt, any n, any alignment) is read once and round_w(theta) (RNE, torch copy_) is
 * stored into bcast[0..nbcast) (n elements of wdt each) — nbcast device copies in one pass.
 * Operands that are all 16-byte aligned take 8-element accesses with a scalar tail, others the
 * scalar path. 0 <= nbcast <= 64 (0: nothing to do). EDT_ERR_ARG for an unsupported dtype pair, a
 * null pointer or a destination that overlaps theta_g. */
int edt_broadcast_theta(const void* theta_g, int gdt, uint64_t n, void* const* bcast, int wdt, int nbcast,
                        void* stream);

/* ---- EDT pairwise merge -------------------------------------------------------------------
 * Replaces EDT_LM/train/crossover.py:150-163 + 166-230 for one child:
 *   B = lerp(0.5, b1, b2)                         (run_linear_merge_5050, in the model dtype wdt)
 *   d = ((m1 - B) + (m2 - B)) / 2 ; grad = -d      (run_sgd, in the base dtype gdt)
 *   SGD(lr, momentum, nesterov).step() with the parent's momentum when has_momentum = 1.
 * Writes the child parameters to theta_out (gdt) and the new momentum buffer in place.
 * The parents' bases b1/b2 and trained weights m1/m2 have dtype wdt. b2 may be NULL: b1 is
 * then the already merged base of dtype gdt (run_sgd called on a given base_model). */
int edt_pair_merge(const void* b1, const void* b2, const void* m1, const void* m2, int wdt,
                   void* theta_out, int gdt, void* momentum, int has_momentum, uint64_t n,
                   double lr, double momentum_coef, int nesterov, void* stream);

/* edt_pair_merge with the inherited momentum read from `momentum_in` (the donor parent's
 * outer_optim.pt buffer, EDT_LM/train/crossover.py:183-219) and the child's written to
 * `momentum_out`: the donor stays intact for the other children it feeds, and no copy of it is
 * made first. momentum_in == momentum_out is edt_pair_merge. */
int edt_pair_merge_to(const void* b1, const void* b2, const void* m1, const void* m2, int wdt,
                      void* theta_out, int gdt, const void* momentum_in, void* momentum_out,
                      int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                      void* stream);

/* Every EDT-LM child of a resident population in ONE launch (EDT_LM/edt_sim.py:244-256: one child
 * per machine from the selected pairs): child c is edt_pair_merge_to(b1[c], b2[c], m1[c], m2[c],
 * out[c], momentum_in[c] -> momentum_out[c], has_momentum[c]) — host arrays of nchildren (<= 16)
 * device pointers; parents repeat across children (a parent feeds ~2). The workgroups of all
 * children for one chunk of elements share an XCD (blockIdx % 8) and run together, so each parent
 * chunk is fetched from HBM once and served from L2 / the Infinity Cache to its other readers.
 * Results are bit-identical to the per-child calls. Outputs must not alias any input. */
int edt_pair_merge_population(const void* const* b1, const void* const* b2, const void* const* m1,
                              const void* const* m2, int wdt, void* const* out, int gdt,
                              const void* const* momentum_in, void* const* momentum_out,
                              const int32_t* has_momentum, int nchildren, uint64_t n, double lr,
                              double momentum_coef, int nesterov, void* stream);

/* lerp(t, v0, v1) = (1-t)*v0 + t*v1 as three rounded ops in compute dtype cdt (= the tensors'
 * dtype for torch, F32 for numpy), stored as out_dt.
 * Replaces EDT_LM/train/crossover.py:50-51 / EDT_RL/crossover.py:46-47 when applied per tensor. */
int edt_lerp(const void* v0, const void* v1, int in_dt, void* out, int out_dt, int cdt,
             uint64_t n, double t, void* stream);

/* ---- SLERP crossover (EDT_RL/crossover.py:11-43, EDT_EVOMERGE/train/crossover.py:14-46) ------
 * Multi-tensor: the parents v0, v1 are flat buffers holding `nseg` tensors; segment s spans
 * [seg_offsets[s], seg_offsets[s+1]). Work is cut into chunks that never cross a segment.
 *
 * edt_slerp_make_chunks (HOST function): fills chunk_desc (3 uint64 per chunk:
 *   start, length, segment) and seg_first_chunk (nseg+1) for chunk length `chunk_elems`
 *   (<= 65536: a chunk's sums are a fixed tree over at most 128 tiles of 512 elements);
 *   returns the chunk count, or the required count (negated - 1) if max_chunks is too small. */
int64_t edt_slerp_make_chunks(const uint64_t* seg_offsets_host, int nseg, uint32_t chunk_elems,
                              uint64_t* chunk_desc_host, int64_t max_chunks,
                              int32_t* seg_first_chunk_host);

/* Chunk-sum tables. Every chunk's fp64 sums are formed in one canonical order (edt_slerp.hip:
 * per-lane FMA chains over 512-element tiles, the wave butterfly, a perfect binary tree over the
 * tiles), written as partial-tree rows: a table of W sums per chunk
 * therefore needs edt_slerp_sums_doubles(W, nchunks) doubles — the chunk rows [nchunks][W] first
 * (what the coefficient passes read and what a caller may copy or all-gather), then the row
 * scratch the sum pass fills and folds into the rows (W = 3: and one flag word at the end). Every
 * `partial` of the pair forms below holds edt_slerp_sums_doubles(3, nchunks) doubles. */
uint64_t edt_slerp_sums_doubles(int width, int64_t nchunks);

/* Pass 1: per-chunk sums  partial[c] = { sum v0^2, sum v1^2, sum v0*v1 }  (fp64). */
int edt_slerp_stats(const void* v0, const void* v1, int in_dt, const uint64_t* chunk_desc,
                    int64_t nchunks, double* partial, void* stream);

/* Per segment: reduce the chunk sums in a fixed order, form the norms, the normalised dot and
 * the blend coefficients coef[2s], coef[2s+1] exactly as the reference's branch does:
 *   |dot| > dot_threshold -> (1-t, t) (lerp);  else (sin((1-t)th)/sin th, sin(t th)/sin th).
 * t: device array of nseg doubles (interpolate_t / global t per key). dot_out (nullable): the
 * fp32 dot per segment. */
int edt_slerp_coef(const double* partial, const int32_t* seg_first_chunk, int nseg,
                   const double* t, double dot_threshold, double eps, float* coef,
                   float* dot_out, void* stream);

/* Pass 2: out = coef0*v0 + coef1*v1 in fp32 (numpy: two rounded products, one rounded sum),
 * stored as out_dt (RN to bf16 when the merged model is bf16, EDT_EVOMERGE/train/crossover.py:142). */
int edt_slerp_blend(const void* v0, const void* v1, int in_dt, void* out, int out_dt,
                    const uint64_t* chunk_desc, int64_t nchunks, const float* coef, void* stream);

/* The three passes above in one call (stats -> coef -> blend), stream-ordered. A
 * segment-grouped variant that re-reads each group from the Infinity Cache measured slower on
 * MI355X (launch count; 87 % of a 7B body's bytes sit in tensors larger than the cache), so the
 * whole-arena form is the one shipped. */
int edt_slerp_merge(const void* v0, const void* v1, int in_dt, void* out, int out_dt,
                    const uint64_t* chunk_desc, int64_t nchunks, const int32_t* seg_first_chunk, int nseg,
                    const double* t, double dot_threshold, double eps, double* partial, float* coef,
                    float* dot_out, void* stream);

/* edt_slerp_merge with a speculative first pass: the chunk sums and, in the same pass, the
 * lerp-branch output (1-t) v0 + t v1 of every segment; the coefficients then flag (redo[s] = 1,
 * nseg int32 of device workspace) the segments whose |dot| <= dot_threshold, and only their
 * chunks are blended again with the SLERP coefficients. Parents of one lineage (fine-tunes of a
 * common base: |dot| > 0.9995 on most tensors, EDT_RL/crossover.py:31-32) are merged in ONE pass
 * over them (2 b_in + b_out per element instead of 4 b_in + b_out); segments that take the SLERP
 * branch cost a second full pass. Outputs, sums and dots are bit-identical to edt_slerp_merge.
 * `out` must not overlap the parents (n elements each). */
int edt_slerp_merge_speculative(const void* v0, const void* v1, int in_dt, void* out, int out_dt,
                                const uint64_t* chunk_desc, int64_t nchunks, const int32_t* seg_first_chunk,
                                int nseg, const double* t, double dot_threshold, double eps, double* partial,
                                float* coef, float* dot_out, int32_t* redo, uint64_t n, void* stream);

/* Tensor-list form of edt_slerp_merge: segment i is its own tensor pair v0_t[i], v1_t[i] and is
 * written to out_t[i] (host arrays of nseg device pointers, each 16-byte aligned; NULL only for
 * empty segments), e.g. two models' state-dict tensors merged straight into a third model's
 * parameters (EDT_EVOMERGE/train/crossover.py:104-146 without the state-dict copies). chunk_desc
 * holds starts RELATIVE to their segment (edt_slerp_make_chunks output minus
 * seg_offsets[segment]). The kernels read the tensors through a DEVICE table of 3 x nseg uint64
 * {v0, v1, out} pointers:
 *   edt_slerp_seg_table   (HOST) validates the arrays (alignment; with `apart`, no output byte
 *                         range [out, out + n*osize) overlaps any parent range — a sorted-span
 *                         check over every tensor, seg_numel = the nseg sizes; r5: without
 *                         `apart` but with seg_numel, an output may be exactly one of its OWN
 *                         parents and must overlap no other tensor's parent or output — the
 *                         two-pass blend would race; r6: seg_numel is required whenever
 *                         nseg > 0 — the checks need the sizes) and writes the
 *                         table's host image (3 x nseg uint64). The caller uploads it once and
 *                         reuses it while the tensors stay where they are: the *_table entries
 *                         below then cost no per-tensor host work per call.
 *   edt_slerp_merge_table / _speculative   edt_slerp_merge / _speculative over the table (the
 *                         speculative one needs a table validated with apart = 1)
 *   edt_slerp_stats_table / edt_slerp_blend_table   the passes alone; blend: redo (nseg int32,
 *                         nullable) restricts it to segments with redo[s] != 0
 *   edt_slerp_merge_list / _list_speculative   the same from host pointer arrays: the table is
 *                         validated and copied into `workspace` (24 bytes per segment, device,
 *                         8-byte aligned) by a stream-ordered copy on every call. edt_slerp_merge_list
 *                         takes no sizes, so its in-place rule (an output exactly its own parent
 *                         or apart from every other tensor) is the caller's to keep; the
 *                         speculative form checks its rule over seg_numel. */
int edt_slerp_seg_table(const void* const* v0_t, const void* const* v1_t, void* const* out_t, int nseg,
                        const uint64_t* seg_numel, int in_dt, int out_dt, int apart, uint64_t* table_host);
int edt_slerp_stats_table(const uint64_t* seg_table, int in_dt, const uint64_t* chunk_desc, int64_t nchunks,
                          double* partial, void* stream);
int edt_slerp_blend_table(const uint64_t* seg_table, int in_dt, int out_dt, const uint64_t* chunk_desc,
                          int64_t nchunks, const float* coef, const int32_t* redo, void* stream);
int edt_slerp_merge_table(const uint64_t* seg_table, int in_dt, int out_dt, const uint64_t* chunk_desc,
                          int64_t nchunks, const int32_t* seg_first_chunk, int nseg, const double* t,
                          double dot_threshold, double eps, double* partial, float* coef, float* dot_out,
                          void* stream);
int edt_slerp_merge_table_speculative(const uint64_t* seg_table, int in_dt, int out_dt, const uint64_t* chunk_desc,
                                      int64_t nchunks, const int32_t* seg_first_chunk, int nseg, const double* t,
                                      double dot_threshold, double eps, double* partial, float* coef,
                                      float* dot_out, int32_t* redo, void* stream);
int edt_slerp_merge_list(const void* const* v0_t, const void* const* v1_t, int in_dt,
                         void* const* out_t, int out_dt, const uint64_t* chunk_desc, int64_t nchunks,
                         const int32_t* seg_first_chunk, int nseg, const double* t,
                         double dot_threshold, double eps, double* partial, float* coef,
                         float* dot_out, void* workspace, uint64_t workspace_bytes, void* stream);

/* edt_slerp_merge_list with edt_slerp_merge_speculative's first pass: the chunk sums and the
 * lerp-branch output of every tensor in one pass over the tensors where they lie; only tensors
 * whose |dot| <= dot_threshold (redo[s] = 1, nseg int32 of device workspace) are blended again.
 * Parents of one lineage cost one pass instead of two. Outputs, sums and dots are bit-identical
 * to edt_slerp_merge_list. No output may overlap any parent tensor (checked over the byte ranges
 * from seg_numel, the nseg sizes on the host: EDT_ERR_ARG, and the two-pass list form takes
 * that case); `partial` as edt_slerp_merge_speculative's (its last double holds the any-redo
 * word). */
int edt_slerp_merge_list_speculative(const void* const* v0_t, const void* const* v1_t, int in_dt,
                                     void* const* out_t, int out_dt, const uint64_t* seg_numel,
                                     const uint64_t* chunk_desc, int64_t nchunks,
                                     const int32_t* seg_first_chunk, int nseg, const double* t,
                                     double dot_threshold, double eps, double* partial, float* coef,
                                     float* dot_out, int32_t* redo, void* workspace, uint64_t workspace_bytes,
                                     void* stream);

/* out = coef0*v0 + coef1*v1 (edt_slerp_blend's math) over the chunks whose segment has
 * redo[s] != 0 only (nseg int32, device): the flat-arena re-blend of selected segments. */
int edt_slerp_blend_segments(const void* v0, const void* v1, int in_dt, void* out, int out_dt,
                             const uint64_t* chunk_desc, int64_t nchunks, const float* coef, const int32_t* redo,
                             void* stream);

/* SLERP children of a resident population (EDT_RL/edt.py:286-299: every selected pair of one
 * generation, EDT_RL/crossover.py:84-135 per child): ONE stats pass over the nmembers (<= 8) flat
 * member arenas forms every parent's squared norm and the dots the children need per chunk, then
 * per child the coefficients (from pairs[2q], pairs[2q+1] = member indices, host array) and the
 * blend into outs[q] (host array of device pointers; no output may alias a member). The stats pass
 * runs per connected component of the children's pair graph (r5, any graph the reference's
 * roulette selection draws): a component of D <= 8 parents forms its D norms and only the dots its
 * children use — the edges of the best cyclic order of the parents (the ring) plus up to 4 chord
 * slots (2 at D = 4, none below) — or, when the children need more dots than that, the same pass
 * in the triangle layout (its Gram upper triangle: the norms and the dots used); each parent is
 * read once either way. `gram`: edt_slerp_population_gram_doubles(nmembers, nchunks) doubles of
 * device workspace (layout internal to this call). Each child's sums,
 * coefficients and output are bit-identical to edt_slerp_merge on (members[i], members[j]).
 * coef: [npairs][nseg][2] floats; dot_out (nullable): [npairs][nseg]. */
uint64_t edt_slerp_population_gram_doubles(int nmembers, int64_t nchunks);
int edt_slerp_population(const void* const* members, int nmembers, int in_dt, const int32_t* pairs, int npairs,
                         void* const* outs, int out_dt, const uint64_t* chunk_desc, int64_t nchunks,
                         const int32_t* seg_first_chunk, int nseg, const double* t, double dot_threshold,
                         double eps, double* gram, float* coef, float* dot_out, void* stream);

/* edt_slerp_population with edt_slerp_merge_speculative's first pass, which also writes every
 * child's lerp-branch output: when every component takes the needed-sums layout and npairs <= 16,
 * one member-major launch per component (each parent read once, every child emitted from the
 * parents' registers: ring-edge children directly, the others from a chord slot or a copy);
 * otherwise — the fallback for graphs the reference's 8-pair selection does not draw: more than 16
 * children, more than 8 distinct parents, a component on the triangle layout, or more distinct
 * chord children than the emit slots — one co-located launch (every child of a chunk on one XCD,
 * shared parents read once).
 * Per child the coefficients flag (redo: [npairs][nseg] int32) the SLERP-branch segments, which
 * one launch blends again (it exits at once when no child needs any).
 * partial: edt_slerp_population_speculative_doubles(npairs, nchunks) doubles of workspace.
 * Outputs must not overlap any member (n elements each). Bit-identical to edt_slerp_merge per
 * child either way. */
uint64_t edt_slerp_population_speculative_doubles(int npairs, int64_t nchunks);
int edt_slerp_population_speculative(const void* const* members, int nmembers, int in_dt, const int32_t* pairs,
                                     int npairs, void* const* outs, int out_dt, const uint64_t* chunk_desc,
                                     int64_t nchunks, const int32_t* seg_first_chunk, int nseg, const double* t,
                                     double dot_threshold, double eps, double* partial, float* coef,
                                     float* dot_out, int32_t* redo, uint64_t n, void* stream);

/* The needed-sums passes of edt_slerp_population as separate entries (r5: the link-balanced sharded
 * population — each rank forms the sums of its chunk range, the table rows are all-gathered, every
 * rank forms every child's coefficients; distributed.ShardedPopulationCrossover). Replaces, across
 * the node's GPUs, the RL master's generation EDT_RL/edt.py:286-299 -> EDT_RL/crossover.py:84-135
 * per child (the dots of EDT_RL/crossover.py:20-29). The table of a
 * generation (pairs over nmembers <= 8 members, nchunks chunks) is ncomp blocks, one per connected
 * component of the children's pair graph: block k at block_off[k] doubles, nchunks rows of
 * block_nt[k] sums (the component's norms and the dots its children use, or its Gram triangle
 * when they need more dots than the slots: D(D+1)/2 columns, the dots no child uses not formed).
 * col_members (nullable, 2 x sum(block_nt) int32): the two members of each column, block after
 * block (-1, -1: an unused slot, its sum not formed). scratch_doubles: the
 * row scratch a pass over up to nchunks chunks needs.
 *   edt_slerp_needed_sums  rows [row0, row0 + nchunks) of every block, over a chunk table of those
 *                          nchunks chunks (starts relative to the member buffers), table_chunks =
 *                          the table's row count; a row is bit-identical to edt_slerp_population's
 *                          sums of that chunk, wherever the chunk's elements lie (16-byte aligned)
 *   edt_slerp_needed_coef  every child's coefficients [npairs][nseg][2] and dots [npairs][nseg]
 *                          (nullable) from the complete table
 *   edt_slerp_blend_children (below) then blends a rank's chunks of every child. */
int edt_slerp_needed_table(const int32_t* pairs, int npairs, int nmembers, int64_t nchunks, uint64_t* block_off,
                           int32_t* block_nt, int32_t* ncomp, int32_t* col_members, uint64_t* table_doubles,
                           uint64_t* scratch_doubles);
int edt_slerp_needed_sums(const void* const* members, int nmembers, int in_dt, const int32_t* pairs, int npairs,
                          const uint64_t* chunk_desc, int64_t nchunks, int64_t table_chunks, int64_t row0,
                          double* table, double* scratch, uint64_t scratch_doubles, void* stream);
int edt_slerp_needed_coef(const double* table, int64_t table_chunks, const int32_t* pairs, int npairs, int nmembers,
                          const int32_t* seg_first_chunk, int nseg, const double* t, double dot_threshold, double eps,
                          float* coef, float* dot_out, void* stream);

/* The plan the two population entries above make for a pair graph (the pairs of
 * EDT_RL/edt.py:268-269's selection), as JSON text into buf (host only, no device work): distinct parents, the form (speculative: "member-major" or "co-located";
 * "two-pass"), and per connected component of the children's pair graph its members, distinct
 * dots, sums per element and stats layout ("needed": the members' norms + the dots the children
 * use; "triangle": every pair). For benches and logs. */
int edt_slerp_population_layout(const int32_t* pairs, int npairs, int nmembers, int speculate, char* buf,
                                int buflen);

/* ---- reference-dot mode (opt-in; EDT_RL/crossover.py:20-31 on the reference host) -------------
 * The default coefficients come from an fp64 dot of the chunk sums (within ~3e-7 of the true
 * cosine). The reference decides its branch from an fp32 dot whose error grows with the tensor
 * (BLAS sdot norms, then numpy's pairwise sum of the normalised products), so near
 * DOT_THRESHOLD the two can take different branches. This mode recomputes, for the flagged
 * segments, the reference's own fp32 dot bit for bit (restated and pinned in oracle/edt_oracle.c:
 * numpy 2.2 with OpenBLAS 0.3.29's SkylakeX sdot; `threads` = OpenBLAS's thread count for sdot
 * on the reference host, 1 on the pinned host) and the coefficients from it:
 *   edt_slerp_refdot_flags  flag[s] = 1 where | |dots[s]| - dot_threshold | <= band (band < 0: all)
 *   edt_slerp_refdot        ref_dot[s] for every flagged segment (flag NULL: all); chunks of the
 *                           plan (chunk_elems, a multiple of 8192); workspace (device, 8-byte
 *                           aligned): edt_slerp_refdot_workspace_bytes(...)
 *   edt_slerp_refdot_coef   coef / dot_out of the flagged segments from ref_dot (the branch and the
 *                           fp32 SLERP coefficients of edt_slerp_coef)
 * Order: edt_slerp_stats -> edt_slerp_coef -> flags -> refdot -> refdot_coef -> edt_slerp_blend.
 * The norms are sequential FMA chains by definition (one workgroup per segment and BLAS thread):
 * a parity mode, tens of ms for a 545M-element tensor. */
uint64_t edt_slerp_refdot_workspace_bytes(int nseg, int64_t nchunks, uint32_t chunk_elems, int threads);
int edt_slerp_refdot_flags(const float* dots, int nseg, double dot_threshold, double band, int32_t* flag,
                           void* stream);
int edt_slerp_refdot(const void* v0, const void* v1, int in_dt, const uint64_t* chunk_desc, int64_t nchunks,
                     const int32_t* seg_first_chunk, int nseg, uint32_t chunk_elems, const int32_t* flag, int threads,
                     double eps, float* ref_dot, void* workspace, uint64_t workspace_bytes, void* stream);
/* edt_slerp_refdot over a tensor-list device table (edt_slerp_seg_table; chunk starts relative). */
int edt_slerp_refdot_table(const uint64_t* seg_table, int in_dt, const uint64_t* chunk_desc, int64_t nchunks,
                           const int32_t* seg_first_chunk, int nseg, uint32_t chunk_elems, const int32_t* flag,
                           int threads, double eps, float* ref_dot, void* workspace, uint64_t workspace_bytes,
                           void* stream);
int edt_slerp_refdot_coef(const float* ref_dot, const int32_t* flag, int nseg, const double* t, double dot_threshold,
                          float* coef, float* dot_out, void* stream);

/* ---- the population SLERP's blends, separately (link-balanced sharded population) -----------
 * edt_slerp_population = edt_slerp_needed_sums (every block, all chunks) + edt_slerp_needed_coef +
 * edt_slerp_blend_children. Split so that the sums of a rank's range of whole chunks (its
 * parameter-index shard of all members, EDT_RL/edt.py:286-299's population spread over the node)
 * can be all-gathered before the coefficients: each chunk's sums are formed by the same kernel in
 * the same order wherever the chunk lives, so the coefficients — and every child — equal
 * edt_slerp_merge's bit for bit.
 *   edt_slerp_blend_children  outs[q] = c0 v_a + c1 v_b over the chunks of chunk_desc (starts
 *                         relative to the member buffers), the segment of each chunk selecting
 *                         coef[q][seg] (nseg = the row length of coef); <= 8 members, <= 16
 *                         children, member-major (each member's tile read once per chunk). */
int edt_slerp_blend_children(const void* const* members, int nmembers, int in_dt, const int32_t* pairs,
                             int npairs, void* const* outs, int out_dt, const uint64_t* chunk_desc,
                             int64_t nchunks, const float* coef, int nseg, void* stream);

/* ---- misc ---- */
const char* edt_last_error(void);
const char* edt_version(void);
/* Diagnostic (not a reference surface): edt_outer_step's exact access pattern on the same
 * operands (theta and momentum read and written, K workers read with the same loads, cache policy
 * and grid) with a trivial body that perturbs theta and momentum by ~1e-30 relative. Its time is
 * the memory-system ceiling of the fused step on the device at hand (bench.py reports both).
 * Operands must be 16-byte aligned. */
int edt_probe_stream(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K, void* momentum,
                     uint64_t n, void* stream);

/* bytes of device memory the kernels above may touch per element, for roofline accounting */
int edt_outer_step_bytes_per_elem(int gdt, int wdt, int K, int with_momentum);

#ifdef __cplusplus
}
#endif
#endif /* EDT_SYNC_H */
