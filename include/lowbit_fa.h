/*
 * lowbit_fa.h - C ABI of liblowbit_fa_hip.so: low-bit FlashAttention-2 forward for MI355X (gfx950).
 *
 * This is the drop-in boundary for the reference's native layer.  The reference binds its native
 * code through two pybind11 modules that take torch tensors:
 *     _qattn  (12 functions, csrc/qattn/pybind.cpp:21-38)   - fused attention
 *     _fused  ( 8 functions, csrc/fused/pybind.cpp:21-33)   - quantisation / pre-processing
 * and, on the path that actually runs, through Triton launches made by Python host wrappers
 * (src/triton/quant_per_block.py:181-248, src/triton/attn_qk_int8_per_block.py:169-238,
 * src/triton/attn_qk_int8_per_block_causal.py:337-437).  The entry points below carry the same
 * information across a plain C boundary: raw device pointers, sizes, element strides, a stream.
 *
 * Conventions (same as the reference's native layer):
 *   - the CALLER allocates every output (csrc/qattn: `o`, src/quant.py:70-85: int8 buffers, scales);
 *   - layouts (HND / NHD) are expressed ONLY through strides, exactly as the Triton host wrappers do
 *     (attn_qk_int8_per_block.py:183-196); strides are in ELEMENTS: {batch, head, sequence};
 *     the last (head_dim) stride must be 1 (src/core.py:288-290);
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream, which is where the reference launches, qk_int_sv_f8_cuda.cu:845); no host sync;
 *   - no process-global mutable state: safe to call concurrently on different devices / streams.  The only state the
 *     library keeps is per calling THREAD: the last error message and the one-shot event pair of
 *     lbfa_profile_next_attn (armed and consumed by the same thread);
 *   - the one-call entry points (lbfa_forward, lbfa_forward_varlen) validate every argument before their first launch: a
 *     call that returns LBFA_EINVAL has enqueued nothing (safe under stream capture);
 *   - return 0 on success, non-zero LBFA_E* on failure; `lbfa_last_error()` returns a thread-local
 *     message (the reference raises through TORCH_CHECK, csrc/utils.cuh:19-37, and
 *     std::invalid_argument for unsupported head_dim/flags, csrc/dispatch_utils.h:23-34).
 *
 * Quantisation granularity is the reference Triton path's: one fp32 scale per 128 query rows
 * (BLKQ) and per 64 key rows (BLKK) (src/triton/quant_per_block.py:182).
 */
#ifndef LOWBIT_FA_H_
#define LOWBIT_FA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBFA_VERSION 200 /* 0.2.0 (see INTEGRATION.md "ABI versions"): + lbfa_absmax; the changes of 0.1.1 (lbfa_attn_fwd[_varlen] refuse a
                            bf16 V - cast it with lbfa_cast_bf16_to_f16 -, *_workspace_bytes without a dtype include the fp16 copy of V) are
                            incompatible with 0.1.0 callers and are versioned as such here */

/* element types */
#define LBFA_F16 0
#define LBFA_BF16 1
#define LBFA_E4M3 2 /* OCP e4m3fn (gfx950 native), only as v_dtype of lbfa_attn_fwd */

/* status codes */
#define LBFA_OK 0
#define LBFA_EINVAL 1   /* bad argument (unsupported head_dim, dtype, null pointer ...) */
#define LBFA_ELAUNCH 2  /* HIP launch / runtime error */

#define LBFA_BLKQ 128 /* query rows per scale   (src/triton/quant_per_block.py:182, attn BLOCK_M :179) */
#define LBFA_BLKK 64  /* key rows per scale     (src/triton/quant_per_block.py:182, attn BLOCK_N :180) */

int lbfa_version(void);

/* Thread-local description of the last failure on this thread ("" if none). */
const char* lbfa_last_error(void);

/*
 * Mean over the sequence of x[B,H,S,D] -> mean_out[B,H,D] (contiguous, same dtype as x).
 * Replaces `km = k.mean(dim=seq_dim, keepdim=True)` (src/core.py:292-293); fp64 accumulation in a
 * fixed order (deterministic): the correctly rounded mean (float64 mean -> fp32 -> storage dtype).
 * workspace: >= lbfa_mean_seq_workspace_bytes(B,H,S,D) bytes of device memory (fp64 partial sums), 16-byte aligned.
 */
size_t lbfa_mean_seq_workspace_bytes(int B, int H, int S, int D);
int lbfa_mean_seq(const void* x, int dtype, void* mean_out, void* workspace, size_t workspace_bytes,
                  int B, int H, int S, int D, const int64_t strides_x[3], void* stream);

/*
 * Per-block symmetric quantisation of x[B,H,S,D] (fp16/bf16) to int8 codes + one fp32 scale per
 * (b, h, block of `blk` rows).  Replaces the two launches of
 * `quant_per_block_int8_kernel` (src/triton/quant_per_block.py:132-178, launched :213-247) and, with
 * qmax = 7, `quant_per_block_int4_unpack_kernel` (:22-71) - one 4-bit-range value per int8 byte:
 *     x' = dtype(x - mean)            (only if mean != NULL; `k = k - km`, :186-187)
 *     xs = fp32(x') * sm_scale ; scale = max(max|xs|, 1e-7) / qmax
 *     code = trunc(xs / scale + 0.5*sign)      (round half away from zero, :174-176)
 * The 1e-7 floor is the CUDA quantiser's (csrc/fused/fused.cu:147); the Triton kernel has none and
 * produces NaN on an all-zero block.  Identical bits whenever max|xs| >= 1e-7.
 *   mean      : [B, H_mean, D] contiguous in x's dtype, or NULL.  H_mean = H / mean_group.
 *   out       : int8, strides_out (elements); scale: [B, H, ceil(S/blk)] contiguous fp32.
 *   rowdot_vec: optional [B, H/rowdot_group, D] (x's dtype).  When non-NULL, rowdot_out[B,H,S] (fp32,
 *               contiguous) receives dtype(sum_d x[b,h,s,d] * vec[b,h/rowdot_group,d]) of the
 *               UN-shifted, un-scaled x: the `lse_correction = q @ km^T` of src/core.py:294-304.
 *   qmax in {127, 7}; blk in {128, 64}; D in {64, 128}.
 */
int lbfa_quant_per_block(const void* x, int dtype, const void* mean, int mean_group, int8_t* out, float* scale,
                         float sm_scale, int qmax, int blk, int B, int H, int S, int D,
                         const int64_t strides_x[3], const int64_t strides_out[3],
                         const void* rowdot_vec, int rowdot_group, float* rowdot_out, void* stream);

/*
 * Per-channel FP8 quantisation of V[B,H,S,D] (fp16/bf16).  Replaces `per_channel_fp8`
 * (src/quant.py:210-291 -> TransposePadPermuteKernel + MeanScaleKernel, csrc/fused/fused.cu:263-428):
 *     v_scale[b,h,d] = max(max_s |v|, 1e-7) / 448 ; v_fp8 = e4m3fn_rn_sat(v * 448 / amax)
 * v_fp8 is written in the device layout lbfa_attn_fwd consumes for v_dtype = LBFA_E4M3:
 * [B, H, ceil(S/64), D, 64] bytes - per 64-key tile, channel-major, keys permuted for the MFMA
 * operand (the reference likewise transposes, pads to 64 and permutes for its mma fragment,
 * fused.cu:288-292; the permutation is a device detail, not API).
 *   v_fp8 bytes required: lbfa_v_fp8_bytes(B,H,S,D).  Padded keys are written as 0.
 */
size_t lbfa_v_fp8_bytes(int B, int H, int S, int D);
int lbfa_quant_v_fp8(const void* v, int dtype, uint8_t* v_fp8, float* v_scale, int B, int H, int S, int D,
                     const int64_t strides_v[3], void* stream);

/*
 * Fused attention forward: O = softmax(dequant(Q K^T)) V, FlashAttention-2 tiling, online softmax in
 * base 2 (sm_scale*log2e is already folded into q_scale by the quantiser).  Replaces
 * `_attn_fwd` (src/triton/attn_qk_int8_per_block.py:69-167), its causal twin
 * (src/triton/attn_qk_int8_per_block_causal.py:82-214), the int4 copies
 * (src/triton/quantization/attn_qk_int4_per_block{,_causal}.py) and, for v_dtype = LBFA_E4M3,
 * `qk_int8_sv_f8_accum_f32_fuse_v_scale_attn*` (csrc/qattn/qk_int_sv_f8_cuda.cu:46-692).
 *   q [B,Hq,Sq,D], k [B,Hkv,Sk,D] : int8 codes (any range within int8: 127 or 7)
 *   v : LBFA_F16 [B,Hkv,Sk,D] with strides_v - as the reference's kernel, which is only ever handed `v.to(float16)`
 *       (src/core.py:307-308); a bf16 V is cast with lbfa_cast_bf16_to_f16 first (the one-call entry points do that
 *       themselves) - or LBFA_E4M3 in the layout of lbfa_quant_v_fp8 (strides_v ignored) together with v_scale [B,Hkv,D].
 *   o : [B,Hq,Sq,D] fp16 or bf16 (o_dtype), strides_o.
 *   lse : NULL, or [B,Hq,Sq] contiguous fp32 receiving log2(l) + m (base-2 domain, exactly what the
 *         reference kernel stores, :164-167; the host converts it, src/core.py:344-350).
 *   q_scale [B,Hq,ceil(Sq/128)], k_scale [B,Hkv,ceil(Sk/64)] contiguous fp32.
 *   is_causal requires Sq == Sk (attn_qk_int8_per_block_causal.py:389).
 *   Keys >= Sk are masked with -inf (the CUDA path's behaviour, csrc/qattn/attn_utils.cuh:327-353; the
 *   Triton kernel lets them into the softmax as zeros, a defect that only shows when Sk % 64 != 0).
 *   D in {64, 128}; Hq % Hkv == 0.
 */
int lbfa_cast_bf16_to_f16(const void* src, void* dst, int B, int H, int S, int D, const int64_t strides_src[3],
                          const int64_t strides_dst[3], void* stream); /* src/core.py:307-308 `v.to(float16)`; D % 8 == 0 */
int lbfa_attn_fwd(const int8_t* q, const int8_t* k, const void* v, int v_dtype, void* o, int o_dtype, float* lse,
                  const float* q_scale, const float* k_scale, const float* v_scale,
                  int B, int Hq, int Hkv, int Sq, int Sk, int D,
                  const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3],
                  const int64_t strides_o[3], int is_causal, void* stream);

/*
 * max |x| of a [B,H,S,D] fp16 / bf16 view (strides {batch, head, seq} in elements, last dim contiguous, D % 8 == 0) into ONE
 * device float `out` (zeroed by the call, on `stream`).  Replaces the reduction of `compute_scale`, the per-tensor statistic of
 * the precision router (src/core.py:1039-1048: `paddle.compat.max(paddle.abs(tensor))`); dividing by 2^(bits-1) - 1 and the
 * thresholds of `select_quantization` (:1051-1063) stay on the host.  Order-independent (integer atomic max): deterministic.
 */
int lbfa_absmax(const void* x, int dtype, float* out, int B, int H, int S, int D, const int64_t strides_x[3], void* stream);

/*
 * Profiling aid: the NEXT fused-attention launch made on this thread (by lbfa_attn_fwd or lbfa_forward) is bracketed by
 * hipEventRecord(start_event) / hipEventRecord(stop_event) on its stream; one-shot.  Both are hipEvent_t passed
 * as void* (NULL clears).  Used by bench.py to time the dominant kernel inside the timed region.
 */
int lbfa_profile_next_attn(void* start_event, void* stop_event);

/*
 * The whole operator in ONE call: smooth-K mean, per-block quantisation of Q and K, (fp8: per-channel V
 * quantisation,) fused attention and the LSE fix-up - the body of `sageattn_qk_int8_pv_fp16_triton`
 * (src/core.py:292-350), of `sageattn_qk_int4_pv_fp16_triton` (q_qmax / k_qmax = 7) and of
 * `sageattn_qk_int8_pv_fp8_cuda` (pv_fp8 = 1) after their argument checks and head-dim padding.  Same kernels
 * and results as calling the entry points above one by one (the host front end uses this one to keep the
 * per-call host overhead at one FFI call and one workspace allocation).
 *   q, k, v : fp16/bf16 (dtype), strides in elements {batch, head, seq}; o same dtype, strides_o.
 *   lse     : NULL, or [B,Hq,Sq] fp32 receiving the NATURAL-log LSE incl. the smooth-K correction
 *             (lse2 / 1.44269504 + (q . km) * sm_scale, src/core.py:344-350).
 *   workspace: >= lbfa_forward_workspace_bytes_dt(..., dtype, ...) bytes, 16-byte aligned, caller-owned scratch (int8 codes,
 *             scales, km, partial sums, fp8 V, the fp16 copy of a bf16 V); contents are undefined
 *             afterwards.  lbfa_forward_workspace_bytes(...) (no dtype) returns the size that is enough for either dtype.
 *   sm_scale: softmax scale (1/sqrt(original head_dim) by default on the host side), a double as in the reference's
 *             Python: the Q quantiser multiplies by fp32(sm_scale * 1.44269504) formed in double
 *             (src/triton/quant_per_block.py:226) - with 4-bit-range codes a 1-ulp difference there flips codes;
 *             q_qmax/k_qmax in {127, 7}.
 *   D       : head dim of q, k, v, o - 64, 128, or ANY multiple of 8 up to 128: the kernels then work on 64 / 128
 *             channels and treat the missing ones as the zero padding of src/core.py:277-287 (never read, never
 *             written), so the host makes no padded copies; results are bit-identical to padding on the host.
 *             (lbfa_forward_varlen likewise; the modular entry points take D in {64, 128} only.)
 *   range   : scores s = q.k * sm_scale * log2(e) of any size with pv_fp8 (the kernel keeps its softmax reference as an exact
 *             product once it passes 2^16); with fp16 P (pv_fp8 = 0) up to |s| < 2^27 - q, k of a few thousand times N(0,1):
 *             beyond it the exponent's one fma `s sc - m` against the rounded reference can overflow fp16 P (rows of NaN), as
 *             in every FlashAttention-2 kernel, lbfa_sdpa_fwd included.
 */
size_t lbfa_forward_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Sk, int D, int pv_fp8, int smooth_k, int return_lse);
size_t lbfa_forward_workspace_bytes_dt(int B, int Hq, int Hkv, int Sq, int Sk, int D, int dtype, int pv_fp8, int smooth_k,
                                       int return_lse);
int lbfa_forward(const void* q, const void* k, const void* v, int dtype, void* o, float* lse, void* workspace,
                 size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int Sk, int D,
                 const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3],
                 const int64_t strides_o[3], double sm_scale, int q_qmax, int k_qmax, int pv_fp8, int is_causal,
                 int smooth_k, void* stream);

/*
 * Un-quantised FlashAttention-2 forward, O = softmax(Q K^T * sm_scale) V, on the same tiling as lbfa_attn_fwd with
 * 16-bit MFMAs for both products in the dtype given: fp16 inputs -> fp16 Q K^T, fp16 P and V; bf16 inputs -> bf16 Q K^T, bf16 P
 * and V (no conversion anywhere, as a bf16 FlashAttention-2 does); fp32 softmax and accumulation.  This is the "FP16" branch of
 * the precision router `sageattn_multi_precision` (src/core.py:1066-1096), which the reference sends to `default_attn`
 * (:46-69 / the framework's SDPA).
 *   q [B,Hq,Sq,D], k / v [B,Hkv,Sk,D], o like q: one dtype (LBFA_F16 / LBFA_BF16), strides {batch, head, seq}.
 *   D: any multiple of 8 up to 128 (as lbfa_forward).  lse: NULL or [B,Hq,Sq] fp32 natural-log LSE.
 */
int lbfa_sdpa_fwd(const void* q, const void* k, const void* v, int dtype, void* o, float* lse,
                  int B, int Hq, int Hkv, int Sq, int Sk, int D,
                  const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3],
                  const int64_t strides_o[3], double sm_scale, int is_causal, void* stream);

/*
 * Attention backward: dq, dk, dv of the dense operators (lbfa_forward with pv_fp8 = 0 or 1, and lbfa_sdpa_fwd).  Additive to
 * ABI 200 (LBFA_VERSION unchanged): callers detect it by looking up the symbol.
 *   Straight-through on the quantiser: P is the forward's own P, recomputed from the scores the forward used (the int8 /
 *   int4-range codes x q_scale x k_scale, regenerated bit for bit by the forward's mean and quantiser kernels; or the 16-bit
 *   Q K^T * sm_scale when q_qmax = 0) and from the LSE the forward returned: P = exp2(s2 - lse2), lse2 = (lse - dtype(q . km)
 *   * sm_scale) * log2(e) (the smooth-K correction of src/core.py:344-350 is taken out again).  With the fp8-PV operator that is
 *   the fp32 P before its e4m3 rounding.  The gradient products use the un-quantised 16-bit tensors (fp16 / bf16 MFMA, fp32
 *   accumulation) and the ORIGINAL K (not K - km):
 *     dV = P^T dO,  dP = dO V^T,  delta_i = sum_d dO_id O_id - dLSE_i,  dS = P o (dP - delta),
 *     dQ = sm_scale dS K,  dK = sm_scale dS^T Q;   GQA: dk / dv of a kv head sum over its Hq / Hkv query heads.
 *   Causal, keys >= Sk and queries >= Sq are masked as in the forward.  No float atomics: every sum is formed in one fixed
 *   order, results are bitwise reproducible run to run.
 *   q, k, v, o, dout : fp16 / bf16 (dtype), 16-byte aligned, strides {batch, head, seq} multiples of 8 elements; o is the
 *                      forward's output, dout the upstream gradient of o.
 *   lse  : [B,Hq,Sq] contiguous fp32, the NATURAL-log LSE the forward returned (lbfa_forward / lbfa_sdpa_fwd with lse != NULL).
 *   dlse : NULL, or [B,Hq,Sq] contiguous fp32 upstream gradient of lse.
 *   dq / dk / dv : outputs in dtype, shaped like q / k / v, any element strides.
 *   D    : 64 or 128 (pad other head dims with zeros, as the forward's results are those of the zero-padded tensors).
 *   sm_scale, q_qmax, k_qmax, is_causal, smooth_k : the forward's arguments; q_qmax = k_qmax = 0 selects the un-quantised
 *          scores of lbfa_sdpa_fwd (smooth_k is then ignored).
 *   workspace: >= lbfa_backward_workspace_bytes(B, Hq, Hkv, Sq, Sk, D, q_qmax, smooth_k) bytes, 16-byte aligned; contents
 *          undefined afterwards.  Every argument is checked before the first launch (LBFA_EINVAL: nothing enqueued).
 *   range: the exponent argument fl(fl(s2 sc) - lse2) and lse2 itself are fp32 values the size of the scores, so P carries a
 *          relative error of about 5 * 2^-24 * max(|s2|, |lse2|) (s2 = q.k * sm_scale * log2(e), in binades) besides its one
 *          rounding to the dtype: the gradient error stays at the dtype's rounding of P and dS up to |s2| ~ 2^11 (fp16) /
 *          2^14 (bf16) and grows linearly beyond (about 2^-8 relative in P at the 2^14..2^15 of randint(-100, 100) inputs
 *          at D = 128, whose saturated softmax leaves gradients at the fp32 residue of dP - delta).  The smooth-K
 *          correction taken out of the LSE is the forward's own, bit for bit: the pre-pass forms dtype(q . km) in the
 *          forward kernels' fp32 order (one dtype ulp of it would move a whole row of P by ulp * sm_scale * log2(e)).
 *          Per-element bound: tests/bwd_reference.py `grad_bound`.
 *          Long rows: P and dS are rounded to the dtype before the gradient MFMAs, and most P of a long diffuse row lie below
 *          the smallest normal fp16 (2^-14; 99.5 % of them at 131072 N(0,1) keys).  The conversion and the MFMA keep fp16
 *          subnormals (tests/test_gpu_backward_long.py::test_mfma_keeps_fp16_subnormals), so such a P carries an absolute
 *          error of at most 2^-25, not its whole value, and fp16 gradient accuracy degrades slowly with row length: measured
 *          rel. L2 error against the float64 restatement at 131072 N(0,1) keys 3.2e-4 ... 3.6e-4 for dq / dk and 1.4e-3 for dv
 *          (non-causal; 2.9e-4 causal), 2.8e-4 ... 3.3e-4 on peaky rows at 65537 and 131072 keys; bf16 2.2e-3 ... 2.6e-3 at every
 *          length tested (its rounding of P and dS dominates).
 *   window: none.  Unlike the forward entry points the backward addresses every operand with 64-bit offsets, so no operand
 *          has a per-(batch, head) 2 GiB window: strides times lengths may exceed it (only the grid sizes are limited).
 */
size_t lbfa_backward_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Sk, int D, int q_qmax, int smooth_k);
int lbfa_backward(const void* q, const void* k, const void* v, const void* o, const void* dout, int dtype, const float* lse,
                  const float* dlse, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                  int B, int Hq, int Hkv, int Sq, int Sk, int D,
                  const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3], const int64_t strides_o[3],
                  const int64_t strides_dout[3], const int64_t strides_dq[3], const int64_t strides_dk[3],
                  const int64_t strides_dv[3], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                  void* stream);

/*
 * Packed variable-length batches (reference: `sageattn_varlen`, src/core.py:356-491).
 *   q [total_q, Hq, D], k / v [total_k, Hkv, D]; sequence b owns tokens [cu_seqlens[b], cu_seqlens[b+1]);
 *   cu_seqlens_* are int32 device arrays of B + 1 entries; strides are in elements {head, token}.
 *   max_seqlen_* must be UPPER BOUNDS of the sequence lengths (they size the grids and the padded scale rows, as in the
 *   reference); a sequence longer than the stated maximum is cut there and nothing is read outside the sized buffers.
 *   Quantisation blocks (128 query / 64 key rows) restart at the start of every sequence.
 *
 * lbfa_quant_per_block_varlen replaces one launch of the varlen `quant_per_block_int8_kernel`
 * (src/triton/quant_per_block_varlen.py:22-72,107-141): scale is [sum_b ceil(len_b/blk), H] with
 * cu_seqlens_scale[b] = number of blocks before sequence b (:92-106).  `mean` (NULL or [H/mean_group, D]) is ONE
 * vector per head shared by all sequences - the reference smooths with k.mean(dim=0) over the packed tokens
 * (src/core.py:452-454) - and is subtracted in the storage dtype as in the dense quantiser.
 *
 * lbfa_attn_fwd_varlen replaces `_attn_fwd` of src/triton/attn_qk_int8_block_varlen.py:94-197 and its causal twin
 * (attn_qk_int8_per_block_causal_varlen.py) with the same scale layout; causal assumes len_q == len_k per sequence.
 * No LSE (the reference returns none).  A sequence with len_k == 0 gets zeros.
 *
 * lbfa_forward_varlen = the whole operator in one call (mean over all tokens, both quantisers, attention) on a
 * caller-owned workspace of lbfa_forward_varlen_workspace_bytes(...) bytes; internally the scales use a padded
 * [B, H, max_blocks] layout, so no cu_seqlens_scale tables are needed.  lbfa_forward_varlen_lse adds the LSE and
 * lbfa_backward_varlen the gradients (below).
 */
int lbfa_quant_per_block_varlen(const void* x, int dtype, const void* mean, int mean_group, int8_t* out, float* scale,
                                const int32_t* cu_seqlens, const int32_t* cu_seqlens_scale, float sm_scale, int qmax,
                                int blk, int B, int max_seqlen, int H, int D, const int64_t strides_x[2],
                                const int64_t strides_out[2], void* stream);
int lbfa_attn_fwd_varlen(const int8_t* q, const int8_t* k, const void* v, int v_dtype, void* o, int o_dtype,
                         const float* q_scale, const float* k_scale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                         const int32_t* cu_seqlens_q_scale, const int32_t* cu_seqlens_k_scale,
                         int B, int Hq, int Hkv, int max_seqlen_q, int max_seqlen_k, int D,
                         const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                         const int64_t strides_o[2], int is_causal, void* stream);
size_t lbfa_forward_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q,
                                           int max_seqlen_k, int D);
size_t lbfa_forward_varlen_workspace_bytes_dt(int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q,
                                              int max_seqlen_k, int D, int dtype);
int lbfa_forward_varlen(const void* q, const void* k, const void* v, int dtype, void* o,
                        const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, void* workspace, size_t workspace_bytes,
                        int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D,
                        const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                        const int64_t strides_o[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                        void* stream);

/*
 * lbfa_forward_varlen with an LSE (additive to ABI 200, LBFA_VERSION unchanged).  Same arguments and workspace query, `o` bit
 * for bit what lbfa_forward_varlen writes, plus
 *   lse : NULL (exactly lbfa_forward_varlen) or [Hq, total_q] contiguous fp32, 4-byte aligned - the layout of FlashAttention-2's
 *         varlen softmax_lse.  Row (h, cu_seqlens_q[b] + i) is the natural-log LSE of query i of sequence b, defined as
 *         lbfa_forward defines it: lse2 / log2(e) + dtype(q . km) * sm_scale with km the ONE mean over all packed keys.  Rows
 *         of a sequence with no keys get -inf; rows in no sequence, or past max_seqlen_q in theirs, are not written.
 */
int lbfa_forward_varlen_lse(const void* q, const void* k, const void* v, int dtype, void* o, float* lse,
                            const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, void* workspace, size_t workspace_bytes,
                            int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D,
                            const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                            const int64_t strides_o[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                            void* stream);

/*
 * Backward of lbfa_forward_varlen (additive to ABI 200): the contract of lbfa_backward applied sequence by sequence.  Sequence b
 * owns query tokens [cu_seqlens_q[b], cu_seqlens_q[b+1]) and key tokens [cu_seqlens_k[b], cu_seqlens_k[b+1]), cut at
 * max_seqlen_q / max_seqlen_k as in the forward; no gradient crosses a sequence boundary.  P is rebuilt from the forward's codes
 * (km over all total_k keys, K by the forward's quantiser, Q as the attention kernel quantises it in-kernel) and from its LSE.
 *   q, k, v, o, dout : as lbfa_forward_varlen's tensors (o its output, dout the upstream gradient), 16-byte aligned, strides
 *                      {head, token} multiples of 8 elements.
 *   lse / dlse : [Hq, total_q] fp32 (lbfa_forward_varlen_lse's lse; dlse NULL or its upstream gradient).
 *   dq / dk / dv : outputs in dtype, shaped like q / k / v, strides {head, token}.  Written completely: tokens in no sequence or
 *                  past the cut get zeros, a query whose sequence has no keys gets dq = 0, keys of a sequence with no queries
 *                  get dk = dv = 0.
 *   q_qmax, k_qmax : 127 or 7 each (the varlen forward has no un-quantised mode).  D : 64 or 128 (the caller pads).
 *   Causal assumes len_q == len_k per sequence (unchecked: cu_seqlens stay on the device).  No float atomics: bitwise
 *   reproducible.  workspace: >= lbfa_backward_varlen_workspace_bytes(...) bytes, 16-byte aligned.  Every argument is checked
 *   before the first launch.
 */
size_t lbfa_backward_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                                            int D, int q_qmax, int smooth_k);
int lbfa_backward_varlen(const void* q, const void* k, const void* v, const void* o, const void* dout, int dtype, const float* lse,
                         const float* dlse, void* dq, void* dk, void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                         void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int total_q, int total_k,
                         int max_seqlen_q, int max_seqlen_k, int D,
                         const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2], const int64_t strides_o[2],
                         const int64_t strides_dout[2], const int64_t strides_dq[2], const int64_t strides_dk[2],
                         const int64_t strides_dv[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                         void* stream);

/*
 * Int8 KV cache and decode attention for short queries (additive to ABI 200, LBFA_VERSION unchanged: look the symbols up).
 *
 * The cache of a batch, all tensors contiguous and caller-owned (capacity a multiple of 64, D in {64, 128}; other head dims are
 * zero-padded by the caller - only the new tokens):
 *   k_codes int8 [B, Hkv, capacity, D]      codes of K - km, one per byte (range 127 or 7)
 *   k_scale fp32 [B, Hkv, capacity / 64]    one scale per 64 keys
 *   v_cache fp16 [B, Hkv, capacity, D]      V as the attention kernels see it (`v.to(float16)`; a bf16 V is cast on append)
 *   k_tail  [B, Hkv, 64, D] storage dtype   raw rows of the OPEN 64-key block (the one the next token falls into)
 *   km      [B, Hkv, D] storage dtype       smooth-K mean, FIXED for the life of the cache, or NULL (no smoothing)
 *   seqlens int32 [B] on the device         valid keys per sequence
 *
 * lbfa_kvcache_append adds the rows k_new / v_new [B, Hkv, T, D] (dtype, strides {batch, head, seq} in elements) of which
 * sequence b takes the first new_lens[b] <= T (new_lens NULL: all T), at positions [seqlens[b], seqlens[b] + new_lens[b]).
 * Afterwards every 64-key block those rows touch holds the codes and the scale lbfa_quant_per_block(dtype(K - km), blk = 64,
 * k_qmax) produces for that block of the concatenated K, bit for bit (1e-7 floor included; the scale of the partial last block
 * comes from the rows present): the open block is re-quantised from k_tail plus the new rows, and k_tail then holds the raw rows
 * of the new open block.  seqlens is READ on the device and NOT advanced: the caller adds new_lens afterwards.  Rows that would
 * pass the capacity are dropped.  Race-free and scheduling-independent for any T (one workgroup owns both ends of the range).
 * km is an input: on the first append the caller fills it with lbfa_mean_seq (all sequences T rows: the mean the dense operators
 * use, so the codes are theirs) or lbfa_kvcache_mean (ragged: storage dtype of the float64 mean over the new_lens[b] valid
 * rows, zeros for an empty sequence).  A softmax row is invariant to any fixed shift of K; lbfa_decode corrects the LSE.
 */
int lbfa_kvcache_mean(const void* k_new, int dtype, const int32_t* new_lens, void* km, int B, int Hkv, int T, int D,
                      const int64_t strides_k[3], void* stream);
int lbfa_kvcache_append(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                        int8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                        int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                        int k_qmax, void* stream);

/*
 * lbfa_decode: O = softmax(dequant(Q K^T)) V of q [B, Hq, Sq, D] (fp16 / bf16, strides_q) over the cache, for
 * M = Sq * (Hq / Hkv) <= 64 query rows per kv head (more: LBFA_EINVAL - such calls belong on lbfa_prefill below; the message names the dense operator).
 *   seqlens[b]    : valid keys of sequence b, the tokens just appended included; max_seqlen_k (1 .. capacity) is a host upper
 *                   bound that sizes the grid, longer sequences are cut there.  seqlens[b] == 0: zeros and LSE -inf.
 *   Q             : quantised inside the kernel, the Sq rows of one (batch, head) as one block with fp32(sm_scale * 1.44269504)
 *                   formed in double: codes and scale bit-identical to lbfa_quant_per_block (blk = 128) on q.
 *   arithmetic    : int8 MFMA scores x q_scale x k_scale, online softmax in base 2, P rounded to fp16, fp16 MFMA against
 *                   v_cache, fp32 accumulation.  Keys >= seqlens[b] are masked with -inf.
 *   is_causal     : bottom-right aligned - query i sees keys < seqlens[b] - Sq + 1 + i (a query that sees none: zeros, -inf).
 *   num_splits    : key slices per sequence, cut at multiples of 64 keys (slice s = tiles [s * tps, (s + 1) * tps) of the
 *                   sequence's ceil(len / 64), tps = ceil(tiles / num_splits)); 0 = lbfa_decode_num_splits(B, Hkv, max_seqlen_k):
 *                   min(ceil(1024 / (B * Hkv)), tiles / 4, 256), at least 1.  One slice writes o directly (one launch); more
 *                   write fp32 partials to the workspace and a second kernel adds them in one fixed order: no atomics, bitwise
 *                   reproducible for a given num_splits.
 *   o             : [B, Hq, Sq, D] in dtype, strides_o.  lse: NULL or [B, Hq, Sq] fp32 natural log, including the smooth-K
 *                   correction dtype(q . km) * sm_scale as lbfa_forward defines it (km NULL: none).
 *   workspace     : >= lbfa_decode_workspace_bytes(..., num_splits) bytes, 16-byte aligned (0 bytes / NULL with one slice).
 *   No 2 GiB window: the cache is addressed with 64-bit offsets.  Every argument is checked before the first launch; the call
 *   only enqueues on `stream`.
 */
int lbfa_decode_num_splits(int B, int Hkv, int max_seqlen_k);
size_t lbfa_decode_workspace_bytes(int B, int Hq, int Hkv, int Sq, int D, int max_seqlen_k, int num_splits);
int lbfa_decode(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);

/*
 * The same cache as a POOL OF PAGES behind one block table per sequence (additive to ABI 200, LBFA_VERSION unchanged: look the
 * symbols up).  All tensors contiguous and caller-owned; page_size a positive multiple of 64, D in {64, 128}:
 *   k_codes     int8  [num_pages, Hkv, page_size, D]         codes of K - km
 *   k_scale     fp32  [num_pages, Hkv, page_size / 64]       one scale per 64 keys
 *   v_cache     fp16  [num_pages, Hkv, page_size, D]         V
 *   block_table int32 [num_slots, max_pages_per_seq], device pages of each sequence; entries past a sequence's last page are
 *                                                            never read
 *   k_tail      [num_slots, Hkv, 64, D] storage dtype        raw rows of the open 64-key block
 *   km          [num_slots, Hkv, D] storage dtype, or NULL   smooth-K mean PER SEQUENCE, fixed while the sequence lives
 *   seqlens     int32 [num_slots], device                    valid keys per sequence
 * Key j of the sequence in slot s lives in page block_table[s, j / page_size] at row j % page_size.  A page never splits a
 * 64-key quantiser block or a 64-key tile of the decode kernel, so both calls do the arithmetic of their contiguous twins in
 * the same order: the same appends give the same codes, scales and V, and the same decode gives the same O and LSE bit for bit
 * (for the same num_splits).
 *   slots : int32 [B] on the device or NULL - row b of the call (of k_new / v_new / new_lens, of q / o / lse) addresses slot
 *           slots[b]; NULL: slot b.  B <= num_slots.  The slots of one append must be distinct (unchecked).
 *   The host cannot check what is on the device: neither kernel ever forms an address from a slot outside [0, num_slots) or a
 *   page outside [0, num_pages).  lbfa_decode_paged CLAMPS the id (a corrupt table gives a wrong answer, not a fault),
 *   lbfa_kvcache_paged_append SKIPS the row / the 64-key block.  This defence is wave-uniform scalar work.
 *
 * lbfa_kvcache_paged_append: the contract of lbfa_kvcache_append.  new_lens is indexed by row of the call; seqlens, k_tail, km
 * and block_table by slot.  The open block is re-quantised from k_tail plus the new rows: codes and scales are bit-identical
 * to the dense quantiser on the concatenated K.  seqlens is read on the device and not advanced.  Rows beyond
 * max_pages_per_seq * page_size are dropped.  The pages of the rows [seqlens[s], seqlens[s] + new_lens[b]) must be in the
 * table before the call.  One workgroup owns both ends of the appended range.
 *
 * lbfa_decode_paged: the contract of lbfa_decode - M = Sq * (Hq / Hkv) <= 64, bottom-right causal alignment, num_splits, the
 * same LSE definition, lbfa_decode_num_splits / lbfa_decode_workspace_bytes (called with B, not num_slots) and the same second
 * kernel over the partials; max_seqlen_k in [1, max_pages_per_seq * page_size].  64-bit offsets everywhere: the pool may
 * exceed 4 GiB.  Every host-visible argument is checked before the first launch (LBFA_EINVAL).
 */
int lbfa_kvcache_paged_append(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                              int8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                              const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T, int D, int num_slots,
                              int num_pages, int page_size, int max_pages_per_seq, const int64_t strides_k[3],
                              const int64_t strides_v[3], int k_qmax, void* stream);
int lbfa_decode_paged(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                      const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, void* o, float* lse,
                      void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages,
                      int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                      const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);

/*
 * Cached prefill: attention of ANY number of queries to the same caches (additive to ABI 200, LBFA_VERSION unchanged: look the
 * symbols up).  lbfa_decode keeps refusing Sq * (Hq / Hkv) > 64; calls at or below that limit belong there.
 *
 * lbfa_prefill: O = softmax(dequant(Q K^T)) V of q [B, Hq, Sq, D] (fp16 / bf16, strides_q) over the contiguous cache, Sq >= 1.
 *   keys          : seqlens[b] valid keys of sequence b, the keys of these queries appended first; max_seqlen_k (1 .. capacity) is
 *                   the host upper bound, longer sequences are cut there.  Keys >= seqlens[b] are masked with -inf and their V
 *                   rows enter as zeros (stale cache rows may hold anything).
 *   q_lens        : int32 [B] on the device, or NULL (all Sq): sequence b owns the first q_lens[b] rows of q[b], the value
 *                   clamped to [0, Sq] on the device.  Rows at or past it are written as zeros with LSE -inf.  The result for
 *                   sequence b equals the call on q[b, :, :q_lens[b]] alone.  The counterpart of new_lens of the append.
 *   Q             : quantised inside the kernel in blocks of 128 rows counted from row 0 of each (batch, query head), the last
 *                   block cut at q_lens[b], its amax taken over its valid rows, with fp32(sm_scale * 1.44269504) formed in
 *                   double: codes and scales bit-identical to lbfa_quant_per_block (blk = 128) on the valid rows; q_qmax in
 *                   {127, 7}.  A cache filled by one uniform append and read with Sq == Sk sees exactly the Q and K codes of
 *                   the dense operator.
 *   arithmetic    : the decode kernel's - scores fp32(int32(q . k)) * q_scale * k_scale, online softmax in base 2 on the exact
 *                   argument s - m, P rounded to fp16, fp16 MFMA against v_cache, fp32 accumulation.
 *   is_causal     : bottom-right aligned - query i of sequence b sees keys < seqlens[b] - q_lens[b] + 1 + i (a query that sees
 *                   none: zeros, -inf).  A Q block skips every 64-key tile wholly past its last row's limit.
 *   lse           : NULL or [B, Hq, Sq] fp32 natural log, including dtype(q . km) * sm_scale as lbfa_decode defines it.
 *   num_splits    : key slices, cut at multiples of 64 keys over the tiles a Q block can see (slice s = tiles [s * tps,
 *                   (s + 1) * tps) of them, tps = ceil(tiles / num_splits)); 0 = lbfa_prefill_num_splits(B, Hq, Sq, max_seqlen_k):
 *                   max(1, min(ceil(512 / (B * Hq * ceil(Sq / 128))), tiles / 4, 256)), tiles = ceil(max_seqlen_k / 64).  One
 *                   slice writes o and lse directly; more write the decode kernel's fp32 partials ([B, Hkv, splits, M, D] and
 *                   [.., M, 4], row hl * Sq + sq, M = Sq * (Hq / Hkv)) and the decode call's second kernel adds them in one
 *                   fixed order: no atomics, bitwise reproducible for a given num_splits.
 *   workspace     : >= lbfa_prefill_workspace_bytes(..., num_splits) bytes, 16-byte aligned (0 bytes / NULL with one slice).
 *   All offsets are 64-bit: no 2 GiB window.  Every host-visible argument is checked before the first launch: LBFA_EINVAL means
 *   nothing was enqueued.
 *   Grid limits (LBFA_EINVAL "grid too large"): B, Hq, Hkv <= 65535; Sq * (Hq / Hkv) and ceil(Sq / 128) * num_splits < 2^24.
 * lbfa_prefill_paged: the same over the pool of pages, with the arguments and the device-side defences of lbfa_decode_paged
 * (slot and page ids are clamped into range: a corrupt table gives a wrong answer, never an address outside the pool; the pool
 * may exceed 4 GiB).  q_lens is indexed by row of the call, seqlens / km / block_table by slot.  Same O and LSE as lbfa_prefill
 * bit for bit for the same num_splits.
 * Not built: a backward through the cache, fp8 PV over the cache, prefix sharing / copy-on-write, Paddle tensors, routing
 * lbfa_decode calls with more than 64 rows here.
 */
int lbfa_prefill_num_splits(int B, int Hq, int Sq, int max_seqlen_k);
size_t lbfa_prefill_workspace_bytes(int B, int Hq, int Hkv, int Sq, int D, int max_seqlen_k, int num_splits);
int lbfa_prefill(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                 const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                 int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                 const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_prefill_paged(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                       const int32_t* seqlens, const int32_t* q_lens, const int32_t* block_table, const int32_t* slots, void* o,
                       float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots,
                       int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits,
                       const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal,
                       void* stream);

/* ---- fp8 V cache: V as e4m3 codes with one scale per key (additive to ABI 200) ------------------------------------------
 * The decode kernel streams 3 D bytes per key and kv head, 2 D of them fp16 V.  With V kept as OCP e4m3fn codes and ONE fp32
 * scale per key and kv head the stream is 2 D + 4 bytes, and the cache takes about two thirds of the memory.  A scale per key
 * depends on nothing but the row itself: a row is written once, never re-quantised, needs no tail buffer and is paged exactly as
 * the codes are.  The K state (k_codes, k_scale, k_tail, km, seqlens) is what it is in the fp16-V cache, bit for bit.
 *
 * Format.  v_cache is uint8 [B, Hkv, capacity, D] (paged: [num_pages, Hkv, page_size, D]), v_scale fp32 [B, Hkv, capacity]
 * (paged: [num_pages, Hkv, page_size], found from the same pool tile as codes and V).  The quantiser of one appended row works on
 * its D channels, all in fp32:
 *     x = fp32(v);  amax = max(max |x|, 1e-7);  scale = amax / 448 (correctly rounded);  code = e4m3fn_rne(x / scale).
 * |x / scale| <= 448 (1 + 2^-23), so no code depends on saturation.  Code and scale of a row never change after they are
 * written: any append schedule gives the state of a one-shot append, bit for bit.
 *
 * What a reader sees is  V^ = fp16_rne(fp32(decode(code)) * scale) : one fp32 multiply and one round-to-nearest-even conversion
 * per element, fp16 subnormals kept.  For finite input |V^ - V| <= (2^-4 + 2^-10) |V| + 2^-10 scale + 2^-24 per element; a bf16
 * magnitude past 65504 becomes inf as it does in the fp16 cache; non-finite V rows are outside the contract and do not disturb
 * other rows.  A read of an fp8 cache equals, bit for bit, the same read of an fp16 cache whose V holds V^, for the same
 * num_splits, contiguous or paged: the tile is turned into V^ on its way into the LDS image, everything behind it is the fp16
 * kernel (rows at or past the length enter as zeros whatever their codes and scales are).
 *
 * Each entry point has the contract, the refusals and the device-side defences of its sibling without the suffix (lengths
 * clamped; slot and page ids clamped for the reads and skipped for the appends; appends clipped at the capacity), the same
 * lbfa_decode_num_splits / lbfa_prefill_num_splits rules and workspace sizes.  The argument lists are the siblings' with v_cache
 * as uint8_t* and v_scale directly behind it.  Two more refusals: a NULL v_scale ("null pointer") and a v_scale that is not
 * 16-byte aligned, both LBFA_EINVAL.
 */
int lbfa_kvcache_append_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                           int8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail, const int32_t* seqlens,
                           int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                           int k_qmax, void* stream);
int lbfa_kvcache_paged_append_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                                 int8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail,
                                 const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T,
                                 int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq,
                                 const int64_t strides_k[3], const int64_t strides_v[3], int k_qmax, void* stream);
int lbfa_decode_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                   const void* km, const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                   int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                   const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_decode_paged_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                         const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* block_table,
                         const int32_t* slots, void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv,
                         int Sq, int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k,
                         int num_splits, const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax,
                         int is_causal, void* stream);
int lbfa_prefill_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                    const void* km, const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace,
                    size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                    const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_prefill_paged_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                          const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* q_lens,
                          const int32_t* block_table, const int32_t* slots, void* o, float* lse, void* workspace,
                          size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages, int page_size,
                          int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                          const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);

/* ---- nibble-packed int4 K cache: two K codes per byte (additive to ABI 200) -----------------------------------------------
 * With k_qmax = 7 the K codes lie in [-7, 7] and still take a byte each in the caches above: as large, as long a stream as int8
 * codes.  The _k4 entry points keep them two to a byte, D / 2 bytes per key and kv head: the decode stream is 2.5 D bytes per key
 * instead of 3 D with fp16 V (_k4), 1.5 D + 4 instead of 2 D + 4 with fp8 V (_k4_v8).
 *
 * Format.  k_codes is uint8 [B, Hkv, capacity, D / 2] (paged: [num_pages, Hkv, page_size, D / 2]).  Byte j of a row holds channel
 * 2 j in bits 0..3 and channel 2 j + 1 in bits 4..7, each nibble the two's-complement 4-bit value of the code the byte cache would
 * hold; the quantiser never produces -8.  A 64-key tile is 32 D contiguous bytes inside one page.  k_scale, k_tail, km, seqlens,
 * v_cache, v_scale, the block table and the re-quantisation of the open 64-key block on each append are exactly the byte cache's: a
 * row is packed from its own codes, so any append schedule gives the state of a one-shot append, bit for bit, and the codes are
 * those of the sibling called with k_qmax = 7.
 *
 * A read of a packed cache equals, bit for bit, the same read of the byte-per-code cache with k_qmax = 7, for the same num_splits,
 * contiguous or paged: the integer score q . k does not depend on the order its channels are added in, and everything behind it
 * is the sibling's kernel.
 *
 * Each entry point has the contract, the refusals and the device-side defences of its sibling without "_k4" (lengths clamped;
 * slot and page ids clamped for the reads and skipped for the appends; appends clipped at the capacity), the same split rules and
 * workspace sizes, and the sibling's argument list with k_codes as uint8_t*.  One more refusal, LBFA_EINVAL before any launch: an
 * append with k_qmax != 7 ("k_qmax must be 7 ..."): the codes must fit a nibble.  k_codes must be 16-byte aligned, as the
 * siblings' (their message).
 */
int lbfa_kvcache_append_k4(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                           uint8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                           int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                           int k_qmax, void* stream);
int lbfa_kvcache_paged_append_k4(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                                 uint8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                                 const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T, int D, int num_slots,
                                 int num_pages, int page_size, int max_pages_per_seq, const int64_t strides_k[3],
                                 const int64_t strides_v[3], int k_qmax, void* stream);
int lbfa_kvcache_append_k4_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                              uint8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail, const int32_t* seqlens,
                              int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                              int k_qmax, void* stream);
int lbfa_kvcache_paged_append_k4_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                                    uint8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail,
                                    const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T,
                                    int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq,
                                    const int64_t strides_k[3], const int64_t strides_v[3], int k_qmax, void* stream);
int lbfa_decode_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                   const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                   int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                   const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_decode_paged_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                         const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, void* o, float* lse,
                         void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages,
                         int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                         const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_decode_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                      const void* km, const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                      int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                      const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_decode_paged_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                            const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* block_table,
                            const int32_t* slots, void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv,
                            int Sq, int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k,
                            int num_splits, const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax,
                            int is_causal, void* stream);
int lbfa_prefill_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                    const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                    int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                    const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_prefill_paged_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                          const int32_t* seqlens, const int32_t* q_lens, const int32_t* block_table, const int32_t* slots, void* o,
                          float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots,
                          int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits,
                          const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal,
                          void* stream);
int lbfa_prefill_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                       const void* km, const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace,
                       size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                       const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);
int lbfa_prefill_paged_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                             const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* q_lens,
                             const int32_t* block_table, const int32_t* slots, void* o, float* lse, void* workspace,
                             size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages, int page_size,
                             int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                             const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOWBIT_FA_H_ */
