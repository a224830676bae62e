// extern "C" entry points of liblowbit_fa_hip.so (declared in include/lowbit_fa.h).
// Argument validation mirrors the reference's checks (src/core.py:269-290, csrc/utils.cuh:19-37,
// csrc/dispatch_utils.h:23-34); failures return a status code and leave a thread-local message.
#include <cstdarg>
#include <cstdio>

#include "lbfa_common.h"

namespace lbfa {
// defined in quant_kernels.hip / attn_fwd.hip
int mean_rows_per_split(int S);
size_t v_fp8_payload_bytes(int B, int H, int S, int D);
hipError_t launch_mean_seq(const void* x, int dtype, void* out, void* ws, int B, int H, int S, int D, int d_valid,
                           const int64_t* st, hipStream_t stream, bool finalize);
hipError_t launch_quant_per_block(const QuantParams& p, int dtype, int D, int blk, hipStream_t stream);
hipError_t launch_quant_v_fp8(const void* v, int dtype, uint8_t* out, float* v_scale, int B, int H, int S, int D,
                              int d_valid, const int64_t* st, hipStream_t stream);
hipError_t launch_attn_fwd(const AttnParams& p, int D, int v_dtype, int o_dtype, int causal, hipStream_t stream);
hipError_t launch_attn_fwd_f16(const AttnParams& p, int D, int dtype, int causal, hipStream_t stream);
hipError_t launch_attn_fwd_qq(const AttnParams& p, int D, int dtype, int v_dtype, int causal, hipStream_t stream);
hipError_t launch_cast_bf16_f16(const void* src, void* dst, int B, int H, int S, int d_valid, const int64_t* ss, const int64_t* ds,
                                hipStream_t stream);
hipError_t launch_absmax(const void* x, int dtype, float* out, int B, int H, int S, int D, const int64_t* st, hipStream_t stream);
// defined in attn_bwd.hip
hipError_t launch_attn_bwd(const BwdParams& p, int dtype, bool quant, bool causal, hipStream_t stream);
// the launchers of the KV-cache kernels (kvcache.hip, attn_decode.hip, attn_prefill.hip) are declared in lbfa_common.h
}  // namespace lbfa

namespace {
thread_local char g_err[512] = "";
thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;  // one-shot, see lbfa_profile_next_attn

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return LBFA_OK;
  return fail(LBFA_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// ---------------------------------------------------------------------------------------------------------------
// one description of an operand and of a problem, dense or packed
// ---------------------------------------------------------------------------------------------------------------
// A tensor as the kernels see it: base pointer + strides in elements {batch, head, seq}, last dim contiguous.  A packed
// [total, H, D] tensor is a dense one with batch stride 0.  p is null when the pointer OR its stride array is missing.
struct Operand {
  const void* p;
  int64_t st[3];
  bool strides_multiple_of(int n) const { return (st[0] | st[1] | st[2]) % n == 0; }
};
Operand dense(const void* p, const int64_t st[3]) { return st ? Operand{p, {st[0], st[1], st[2]}} : Operand{nullptr, {0, 0, 0}}; }
Operand packed(const void* p, const int64_t st[2]) { return st ? Operand{p, {0, st[0], st[1]}} : Operand{nullptr, {0, 0, 0}}; }
bool aligned(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
bool aligned(const Operand& t, unsigned n, int stride_multiple) { return aligned(t.p, n) && t.strides_multiple_of(stride_multiple); }

// head dims the one-call operators take directly: the kernels work on 64 / 128 channels and treat the rest as the
// zero padding of src/core.py:277-287 (never read, never written)
bool head_dim_ok(int D) { return D >= 8 && D <= 128 && D % 8 == 0; }
int padded_head_dim(int D) { return D <= 64 ? 64 : 128; }

struct Shape {
  int B, Hq, Hkv, Sq, Sk;      // packed batch: Sq / Sk are the longest sequences
  int total_q, total_k;        // tokens of a packed batch (0: dense, or not known to the entry point)
  int Dg, D;                   // head dim of the caller's tensors / of the kernels (Dg zero-padded to 64 or 128)
  const int32_t *cu_q, *cu_k;  // packed batch: sequence b owns tokens [cu[b], cu[b + 1])
  bool is_packed;
  bool empty() const { return B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || Sk <= 0; }  // the totals are the entry point's to check
  int nQ() const { return (Sq + LBFA_BLKQ - 1) / LBFA_BLKQ; }
  int nK() const { return (Sk + LBFA_BLKK - 1) / LBFA_BLKK; }
  size_t rows_q() const { return is_packed ? (size_t)total_q : (size_t)B * Sq; }
  size_t rows_k() const { return is_packed ? (size_t)total_k : (size_t)B * Sk; }
  // the smooth-K mean is per batch entry, and over ALL tokens of a packed batch (k.mean(dim=0), src/core.py:453)
  int mean_batch() const { return is_packed ? 1 : B; }
  int mean_rows() const { return is_packed ? total_k : Sk; }
  // workspace tensor of H heads in the layout of the problem: [B, H, S, D] or [total, H, D]
  Operand contiguous(const void* p, int H, int S) const {
    return is_packed ? Operand{p, {0, D, (int64_t)H * D}} : Operand{p, {(int64_t)H * S * D, (int64_t)S * D, D}};
  }
};
Shape dense_shape(int B, int Hq, int Hkv, int Sq, int Sk, int D) {
  return Shape{B, Hq, Hkv, Sq, Sk, 0, 0, D, padded_head_dim(D), nullptr, nullptr, false};
}
// total_q / total_k = 0 where the entry point is not told them (lbfa_attn_fwd_varlen)
Shape packed_shape(int B, int Hq, int Hkv, int total_q, int total_k, int max_q, int max_k, int D, const int32_t* cu_q, const int32_t* cu_k) {
  return Shape{B, Hq, Hkv, max_q, max_k, total_q, total_k, D, padded_head_dim(D), cu_q, cu_k, true};
}

// ---------------------------------------------------------------------------------------------------------------
// one set of checks; `who` is the entry point's name in its messages.  0 = passed.
// ---------------------------------------------------------------------------------------------------------------
int check_dtype(int dtype) {
  return dtype == LBFA_F16 || dtype == LBFA_BF16 ? 0 : fail(LBFA_EINVAL, "Input tensors must be in dtype of float16 or bfloat16");
}
// `padded`: the one-call operators pad 8, 16 .. 128 themselves; the modular entry points take what the kernels run on
int check_head_dim(int D, bool padded) {
  return (padded ? head_dim_ok(D) : D == 64 || D == 128) ? 0 : fail(LBFA_EINVAL, "Unsupported head_dim: %d", D);
}
// head dim and extent of one [B, H, S, D] tensor (`what`: "tensor", or "batch" for a packed one with S = max_seqlen)
int check_bhsd(const char* what, int B, int H, int S, int D) {
  if (B > 0 && H > 0 && S > 0 && (D == 64 || D == 128)) return 0;
  return fail(LBFA_EINVAL, "Unsupported head_dim: %d (or empty %s %dx%dx%d)", D, what, B, H, S);
}
int check_gqa(int Hq, int Hkv) {
  return Hq % Hkv == 0 ? 0 : fail(LBFA_EINVAL, "num_qo_heads (%d) must be divisible by num_kv_heads (%d)", Hq, Hkv);
}
int check_causal(int is_causal, int Sq, int Sk) {
  return !is_causal || Sq == Sk ? 0 : fail(LBFA_EINVAL, "qo_len and kv_len must be equal for causal attention");
}
int check_qmax(const char* who, const char* name, int qmax) {
  return qmax == 127 || qmax == 7 ? 0 : fail(LBFA_EINVAL, "%s: %s must be 127 (int8) or 7 (int4 range), got %d", who, name, qmax);
}
int check_input16(const char* who, const char* name, const Operand& t) {
  return aligned(t, 16, 8) ? 0 : fail(LBFA_EINVAL, "%s: %s must be 16-byte aligned with strides that are multiples of 8 elements", who, name);
}
int check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
  if (workspace_bytes < need) return fail(LBFA_EINVAL, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  return aligned(workspace, 16) ? 0 : fail(LBFA_EINVAL, "%s: workspace must be 16-byte aligned", who);
}
int check_attn_grid(const char* who, const Shape& s) {
  return (int64_t)s.B * s.Hq * s.nQ() <= 0x7fffffffLL ? 0 : fail(LBFA_EINVAL, "%s: grid too large", who);
}
// 32-bit buffer offsets: the window of one (batch, head) - or of one sequence - must stay below 2 GiB.  It spans `rows` rows
// and `ahead` rows of tile look-ahead at `seq_stride` elements, plus one row of D elements, of `elem_bytes` each.
bool window_ok(int64_t rows, int64_t ahead, int64_t seq_stride, int elem_bytes, int D) {
  return elem_bytes * ((rows + ahead) * seq_stride + D) <= 0x7fffffffLL;
}
constexpr int kAheadQ = LBFA_BLKQ, kAheadK = 2 * LBFA_BLKK;
// e4m3 V (lbfa_quant_v_fp8) has no strides: tiles [.., D, 64], (Sk + 128) D bytes with no row after them
bool fp8_v_window_ok(int Sk, int D) { return window_ok(Sk, kAheadK - 1, D, 1, D); }

// ---------------------------------------------------------------------------------------------------------------
// workspace layouts: members are offsets, each aligned to 256 bytes; an absent member takes no room
// ---------------------------------------------------------------------------------------------------------------
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Bump {
  size_t used = 0;
  size_t take(size_t n) { const size_t at = used; used += align256(n); return at; }
};
// The PV product of the int8 operators runs on fp16 MFMAs (the reference casts, src/core.py:307-308): a bf16 V is cast once, in a
// pre-pass, into the workspace (4 bytes per element of HBM traffic: 1..6 % of the operator from S = 4K up; converting the tiles on
// their way into LDS instead cost the attention kernel 9..10 % and 25..56 spilled registers).
bool v_cast_prepass(int dtype, int pv_fp8) { return dtype == LBFA_BF16 && !pv_fp8; }

// one-call forward.  Q is quantised inside the attention kernel: no codes, scales or lse-correction buffers for it.
struct FwdLayout {
  size_t km, part, k8, ks, v8, vs, v16, total;
};
FwdLayout fwd_layout(const Shape& s, int pv_fp8, int dtype) {
  FwdLayout L;
  Bump ws;
  const size_t k_elems = s.rows_k() * s.Hkv * s.D;
  L.km = ws.take((size_t)s.mean_batch() * s.Hkv * s.D * 2);
  L.part = ws.take(lbfa_mean_seq_workspace_bytes(s.mean_batch(), s.Hkv, s.mean_rows(), s.D));
  L.k8 = ws.take(k_elems);
  L.ks = ws.take((size_t)s.B * s.Hkv * s.nK() * 4);
  L.v8 = ws.take(pv_fp8 ? lbfa_v_fp8_bytes(s.B, s.Hkv, s.Sk, s.D) : 0);
  L.vs = ws.take(pv_fp8 ? (size_t)s.B * s.Hkv * s.D * 4 : 0);
  L.v16 = ws.take(v_cast_prepass(dtype, pv_fp8) ? k_elems * 2 : 0);  // fp16 copy of a bf16 V, in the layout of the K codes
  L.total = ws.used;
  return L;
}
// backward: the forward's codes and scales of Q and K (quantised operators), lse2 / delta [rows_q per head]
struct BwdLayout {
  size_t km, part, q8, qs, k8, ks, lse2, delta, total;
};
BwdLayout bwd_layout(const Shape& s, bool quant, int smooth_k) {
  BwdLayout L;
  Bump ws;
  const bool sm = quant && smooth_k;
  L.km = ws.take(sm ? (size_t)s.mean_batch() * s.Hkv * s.D * 2 : 0);
  L.part = ws.take(sm ? lbfa_mean_seq_workspace_bytes(s.mean_batch(), s.Hkv, s.mean_rows(), s.D) : 0);
  L.q8 = ws.take(quant ? s.rows_q() * s.Hq * s.D : 0);
  L.qs = ws.take(quant ? (size_t)s.B * s.Hq * s.nQ() * 4 : 0);
  L.k8 = ws.take(quant ? s.rows_k() * s.Hkv * s.D : 0);
  L.ks = ws.take(quant ? (size_t)s.B * s.Hkv * s.nK() * 4 : 0);
  L.lse2 = ws.take(s.rows_q() * s.Hq * 4);
  L.delta = ws.take(s.rows_q() * s.Hq * 4);
  L.total = ws.used;
  return L;
}

// ---------------------------------------------------------------------------------------------------------------
// the stages the entry points are made of: a call description, its checks, its launch.  The modular entry points run
// check + launch of one stage; the one-call operators check every stage they will run, then launch them in order.
// ---------------------------------------------------------------------------------------------------------------
struct MeanCall {
  Operand x;
  int dtype;
  void *out, *ws;
  size_t ws_bytes;
  int B, H, S, D, d_valid;
  bool finalize;  // false: the K quantiser adds the partial sums itself (QuantCall::mean_partial)
};
int check_mean(const MeanCall& c) {
  if (!c.x.p || !c.out || !c.ws) return fail(LBFA_EINVAL, "lbfa_mean_seq: null pointer");
  if (int st = check_bhsd("tensor", c.B, c.H, c.S, c.D)) return st;
  if (int st = check_dtype(c.dtype)) return st;
  if (c.ws_bytes < lbfa_mean_seq_workspace_bytes(c.B, c.H, c.S, c.D)) return fail(LBFA_EINVAL, "lbfa_mean_seq: workspace too small");
  return check_input16("lbfa_mean_seq", "x", c.x);
}
int run_mean(const MeanCall& c, hipStream_t stream) {
  g_err[0] = 0;
  return check_hip(lbfa::launch_mean_seq(c.x.p, c.dtype, c.out, c.ws, c.B, c.H, c.S, c.D, c.d_valid, c.x.st, stream, c.finalize),
                   "lbfa_mean_seq launch");
}

// per-block quantiser of one [B, H, S, D] tensor, or of a packed one (S = the longest sequence)
struct QuantCall {
  const char* who;  // in messages; a dense call is always "lbfa_quant_per_block", whichever entry point makes it
  Operand x, out;
  float* scale;
  int dtype;
  const void* mean;  // [B, H / mean_group, D] (packed: one [H / mean_group, D] set) or null
  int mean_group;
  float sm_scale;
  int qmax, blk, B, H, S, D, d_valid;
  // packed batch: token offsets; cu_scale = the reference's packed scale table [sum_blocks, H], null = padded [B, H, max_blocks];
  // cut: lengths cut at S, as the attention kernel cuts them at max_seqlen_q
  bool is_packed;
  const int32_t *cu_seqlens, *cu_scale;
  bool cut;
  // dense only.  rowdot_out [B,H,S] = x . rowdot_vec; fused last step of the mean: `mean` is then the OUTPUT buffer km is stored to
  const void* rowdot_vec;
  int rowdot_group;
  float* rowdot_out;
  const double* mean_partial;
  int mean_nsplit;
};
int check_quant(const QuantCall& c) {
  const char* who = c.who;
  if (!c.x.p || !c.out.p || !c.scale || (c.is_packed && !c.cu_seqlens)) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (int st = check_bhsd(c.is_packed ? "batch" : "tensor", c.B, c.H, c.S, c.D)) return st;
  if (int st = check_dtype(c.dtype)) return st;
  if (int st = check_qmax(who, "qmax", c.qmax)) return st;
  if (c.blk != 128 && c.blk != 64) return fail(LBFA_EINVAL, "%s: blk must be 128 or 64, got %d", who, c.blk);
  if (c.mean && (c.mean_group <= 0 || c.H % c.mean_group != 0)) return fail(LBFA_EINVAL, "%s: bad mean_group %d for H=%d", who, c.mean_group, c.H);
  if (c.rowdot_vec && (!c.rowdot_out || c.rowdot_group <= 0 || c.H % c.rowdot_group != 0))
    return fail(LBFA_EINVAL, "%s: rowdot_vec needs rowdot_out and a rowdot_group dividing H", who);
  if (int st = check_input16(who, "x", c.x)) return st;
  return aligned(c.out, 8, 8) ? 0 : fail(LBFA_EINVAL, "%s: out must be 8-byte aligned with strides that are multiples of 8", who);
}
int run_quant(const QuantCall& c, hipStream_t stream) {
  lbfa::QuantParams p{};
  p.x = (const unsigned short*)c.x.p;
  p.mean = (const unsigned short*)c.mean;
  p.out = (int8_t*)const_cast<void*>(c.out.p);
  p.scale = c.scale;
  p.rowdot_vec = (const unsigned short*)c.rowdot_vec;
  p.rowdot_out = c.rowdot_out;
  p.xb = c.x.st[0]; p.xh = c.x.st[1]; p.xs = c.x.st[2];
  p.ob = c.out.st[0]; p.oh = c.out.st[1]; p.os = c.out.st[2];
  p.sm_scale = c.sm_scale;
  p.qmax = (float)c.qmax;
  p.B = c.B; p.H = c.H; p.S = c.S;
  p.nblk = (c.S + c.blk - 1) / c.blk;  // packed: grid extent; blocks past a sequence's end exit at once
  p.mean_group = c.mean ? c.mean_group : 1;
  p.rowdot_group = c.rowdot_vec ? c.rowdot_group : 1;
  if (c.cu_scale) { p.scale_b = c.H; p.scale_h = 1; p.scale_blk = c.H; }                // [sum_blocks, H]
  else { p.scale_b = (int64_t)c.H * p.nblk; p.scale_h = p.nblk; p.scale_blk = 1; }      // [B, H, nblk]
  p.cu_seqlens = c.cu_seqlens; p.cu_scale = c.cu_scale;
  p.mean_b = c.is_packed ? 0 : 1;
  p.d_valid = c.d_valid;
  p.mean_partial = c.mean ? c.mean_partial : nullptr;
  p.mean_out = c.mean_partial ? (unsigned short*)const_cast<void*>(c.mean) : nullptr;
  p.mean_nsplit = c.mean_nsplit;
  p.mean_S = c.is_packed ? 0 : c.S;
  p.s_cap = c.cut ? c.S : 0x7fffffff;
  g_err[0] = 0;
  return check_hip(lbfa::launch_quant_per_block(p, c.dtype, c.D, c.blk, stream), c.is_packed ? c.who : "lbfa_quant_per_block launch");
}
// what every quantiser call states; a dense one.  A packed batch adds is_packed and its offset tables.
QuantCall quant_call(const char* who, const Operand& x, const Operand& out, float* scale, int dtype, const void* mean, int mean_group,
                     float sm_scale, int qmax, int blk, int B, int H, int S, int D, int d_valid) {
  QuantCall c{};
  c.who = who; c.x = x; c.out = out; c.scale = scale; c.dtype = dtype;
  c.mean = mean; c.mean_group = mean_group; c.sm_scale = sm_scale; c.qmax = qmax; c.blk = blk;
  c.B = B; c.H = H; c.S = S; c.D = D; c.d_valid = d_valid;
  c.rowdot_group = 1;
  return c;
}
// The quantisers of the one-call operators and of the backward: K (64-row blocks, km subtracted first when smoothing) or
// Q (128-row blocks, sm_scale * log2(e) folded in), codes [B,H,S,D] / [total,H,D] and padded scales in the workspace.
// `packed_who`: the name in the messages of a packed batch.
QuantCall workspace_quant_call(const char* packed_who, const Shape& s, bool is_q, const Operand& x, int dtype, const void* mean,
                               void* codes, float* scale, float sm_scale, int qmax) {
  const int H = is_q ? s.Hq : s.Hkv, S = is_q ? s.Sq : s.Sk;
  QuantCall c = quant_call(s.is_packed ? packed_who : "lbfa_quant_per_block", x, s.contiguous(codes, H, S), scale, dtype, mean, 1,
                           sm_scale, qmax, is_q ? LBFA_BLKQ : LBFA_BLKK, s.B, H, S, s.D, s.Dg);
  c.is_packed = s.is_packed;
  c.cu_seqlens = is_q ? s.cu_q : s.cu_k;
  c.cut = s.is_packed && is_q;  // as the attention kernel's in-kernel Q quantiser cuts
  return c;
}
MeanCall k_mean_call(const Shape& s, const Operand& k, int dtype, void* km, void* part, bool finalize) {
  const int mb = s.mean_batch(), ms = s.mean_rows();
  return MeanCall{k, dtype, km, part, lbfa_mean_seq_workspace_bytes(mb, s.Hkv, ms, s.D), mb, s.Hkv, ms, s.D, s.Dg, finalize};
}

int check_v_fp8(const Operand& v, int dtype, const void* v_fp8, const void* v_scale, int B, int H, int S, int D) {
  if (!v.p || !v_fp8 || !v_scale) return fail(LBFA_EINVAL, "lbfa_quant_v_fp8: null pointer");
  if (int st = check_bhsd("tensor", B, H, S, D)) return st;
  if (int st = check_dtype(dtype)) return st;
  return aligned(v, 16, 8) && aligned(v_fp8, 16) ? 0
         : fail(LBFA_EINVAL, "lbfa_quant_v_fp8: v / v_fp8 must be 16-byte aligned, strides multiples of 8 elements");
}
int run_v_fp8(const Operand& v, int dtype, uint8_t* v_fp8, float* v_scale, int B, int H, int S, int D, int d_valid, hipStream_t stream) {
  g_err[0] = 0;
  return check_hip(lbfa::launch_quant_v_fp8(v.p, dtype, v_fp8, v_scale, B, H, S, D, d_valid, v.st, stream), "lbfa_quant_v_fp8 launch");
}

// ---------------------------------------------------------------------------------------------------------------
// one builder per parameter block
// ---------------------------------------------------------------------------------------------------------------
// Everything the attention kernels share: a raw base-2 LSE (what the reference kernel stores), padded scale tables
// [B,Hq,nQ] / [B,Hkv,nK], Q given as codes.  The call sites below state only what distinguishes them.
lbfa::AttnParams attn_params(const Shape& s, const Operand& q, const Operand& k, const Operand& v, const Operand& o,
                             const float* q_scale, const float* k_scale, const float* v_scale, float* lse) {
  lbfa::AttnParams p{};
  p.q = (const int8_t*)q.p; p.k = (const int8_t*)k.p; p.v = v.p; p.o = const_cast<void*>(o.p); p.lse = lse;
  p.q_scale = q_scale; p.k_scale = k_scale; p.v_scale = v_scale;
  p.qb = q.st[0]; p.qh = q.st[1]; p.qs = q.st[2];
  p.kb = k.st[0]; p.kh = k.st[1]; p.ks = k.st[2];
  p.vb = v.st[0]; p.vh = v.st[1]; p.vs = v.st[2];
  p.ob = o.st[0]; p.oh = o.st[1]; p.os = o.st[2];
  p.B = s.B; p.Hq = s.Hq; p.Hkv = s.Hkv; p.Sq = s.Sq; p.Sk = s.Sk;
  p.nQ = s.nQ(); p.nK = s.nK();
  p.group = s.Hq / s.Hkv;
  p.lse_scale = 1.0f;
  p.qsc_b = (int64_t)s.Hq * p.nQ; p.qsc_h = p.nQ; p.qsc_blk = 1;
  p.ksc_b = (int64_t)s.Hkv * p.nK; p.ksc_h = p.nK; p.ksc_blk = 1;
  p.cu_q = s.cu_q; p.cu_k = s.cu_k;
  p.d_valid = s.Dg;
  p.q_qmax = 127.f;
  return p;
}
// natural-log LSE (src/core.py:347), plus corr_scale * the smooth-K correction (src/core.py:344-350) where one is formed
void natural_log_lse(lbfa::AttnParams& p, double corr_scale) {
  p.lse_scale = 1.0f / 1.44269504f;
  p.lse_corr_scale = (float)corr_scale;
}
// Q arrives as fp16 / bf16 and is quantised by the attention kernel itself (each workgroup its own 128-row block: same codes
// and scales as lbfa_quant_per_block, sm_scale * log2(e) folded in, src/triton/quant_per_block.py:226), as is the LSE
// correction q . km when km is given
void quantise_q_in_kernel(lbfa::AttnParams& p, double sm_scale, int q_qmax, const void* km) {
  p.q_sm_scale = (float)(sm_scale * 1.44269504);  // ONE rounding of the double product, as the reference's kernel argument
  p.q_qmax = (float)q_qmax;
  p.q_dot_vec = (const unsigned short*)km;
}

// in: q, k, v, o, dout; grad: dq, dk, dv.  The forward's codes are added by the caller when the operator is quantised.
lbfa::BwdParams bwd_params(const Shape& s, const Operand (&in)[5], const Operand (&grad)[3], const float* lse, const float* dlse,
                           float* lse2, float* delta, double sm_scale) {
  lbfa::BwdParams p{};
  p.q = (const unsigned short*)in[0].p; p.k = (const unsigned short*)in[1].p; p.v = (const unsigned short*)in[2].p;
  p.o = (const unsigned short*)in[3].p; p.dout = (const unsigned short*)in[4].p;
  p.dq = (unsigned short*)const_cast<void*>(grad[0].p); p.dk = (unsigned short*)const_cast<void*>(grad[1].p);
  p.dv = (unsigned short*)const_cast<void*>(grad[2].p);
  p.lse = lse; p.dlse = dlse;
  p.lse2 = lse2; p.delta = delta;
  p.qb = in[0].st[0]; p.qh = in[0].st[1]; p.qs = in[0].st[2];
  p.kb = in[1].st[0]; p.kh = in[1].st[1]; p.ks = in[1].st[2];
  p.vb = in[2].st[0]; p.vh = in[2].st[1]; p.vs = in[2].st[2];
  p.ob = in[3].st[0]; p.oh = in[3].st[1]; p.os = in[3].st[2];
  p.db = in[4].st[0]; p.dh = in[4].st[1]; p.ds = in[4].st[2];
  p.dqb = grad[0].st[0]; p.dqh = grad[0].st[1]; p.dqs = grad[0].st[2];
  p.dkb = grad[1].st[0]; p.dkh = grad[1].st[1]; p.dks = grad[1].st[2];
  p.dvb = grad[2].st[0]; p.dvh = grad[2].st[1]; p.dvs = grad[2].st[2];
  p.B = s.B; p.Hq = s.Hq; p.Hkv = s.Hkv; p.Sq = s.Sq; p.Sk = s.Sk; p.D = s.D;
  p.nQ = s.nQ(); p.nK = s.nK();
  p.group = s.Hq / s.Hkv;
  p.sm_scale = (float)sm_scale;
  p.qk_scale = (float)(sm_scale * 1.44269504);  // as lbfa_sdpa_fwd
  p.corr_scale = (float)sm_scale;               // as lbfa_forward's LSE fix-up
  p.cu_q = s.cu_q; p.cu_k = s.cu_k;
  p.total_q = s.total_q; p.total_k = s.total_k;
  return p;
}

// launches one of the three attention kernels, bracketed by the caller's events when a profile request is pending
enum class AttnKernel { kCodes, kQuantiseQ, kF16 };  // int8 Q codes given / Q quantised in the kernel / un-quantised Q and K
hipError_t launch_attention(AttnKernel kernel, const lbfa::AttnParams& p, int D, int v_dtype, int o_dtype, int causal, hipStream_t stream) {
  const hipEvent_t e0 = g_prof_start, e1 = g_prof_stop;
  g_prof_start = g_prof_stop = nullptr;
  g_err[0] = 0;
  if (e0) (void)hipEventRecord(e0, stream);
  const hipError_t err = kernel == AttnKernel::kF16         ? lbfa::launch_attn_fwd_f16(p, D, o_dtype, causal, stream)
                         : kernel == AttnKernel::kQuantiseQ ? lbfa::launch_attn_fwd_qq(p, D, o_dtype, v_dtype, causal, stream)
                                                            : lbfa::launch_attn_fwd(p, D, v_dtype, o_dtype, causal, stream);
  if (e1) (void)hipEventRecord(e1, stream);
  return err;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// The C ABI.  The rule every entry point follows: EVERY check comes before the FIRST launch, those of the stages a one-call
// operator is about to run included.  A call that returns LBFA_EINVAL has enqueued nothing (no wasted work, no stray nodes
// in a stream capture the caller believes failed).
// ---------------------------------------------------------------------------------------------------------------
extern "C" {

int lbfa_profile_next_attn(void* start_event, void* stop_event) {
  g_prof_start = (hipEvent_t)start_event;
  g_prof_stop = (hipEvent_t)stop_event;
  return LBFA_OK;
}

int lbfa_version(void) { return LBFA_VERSION; }

const char* lbfa_last_error(void) { return g_err; }

int lbfa_absmax(const void* x, int dtype, float* out, int B, int H, int S, int D, const int64_t strides_x[3], void* stream) {
  const Operand t = dense(x, strides_x);
  if (!t.p || !out) return fail(LBFA_EINVAL, "lbfa_absmax: null pointer");
  if (B <= 0 || H <= 0 || S <= 0 || D <= 0 || D % 8 != 0) return fail(LBFA_EINVAL, "lbfa_absmax: empty tensor or head_dim %d not a multiple of 8", D);
  if (int st = check_dtype(dtype)) return st;
  if (int st = check_input16("lbfa_absmax", "x", t)) return st;
  g_err[0] = 0;
  return check_hip(lbfa::launch_absmax(x, dtype, out, B, H, S, D, t.st, (hipStream_t)stream), "lbfa_absmax launch");
}

size_t lbfa_mean_seq_workspace_bytes(int B, int H, int S, int D) {
  if (B <= 0 || H <= 0 || S <= 0 || D <= 0) return 0;
  const int rps = lbfa::mean_rows_per_split(S);
  const size_t nsplit = (size_t)(S + rps - 1) / rps;
  return (size_t)B * H * nsplit * D * sizeof(double);
}

int lbfa_mean_seq(const void* x, int dtype, void* mean_out, void* workspace, size_t workspace_bytes,
                  int B, int H, int S, int D, const int64_t strides_x[3], void* stream) {
  const MeanCall c{dense(x, strides_x), dtype, mean_out, workspace, workspace_bytes, B, H, S, D, D, true};
  if (int st = check_mean(c)) return st;
  return run_mean(c, (hipStream_t)stream);
}

int lbfa_quant_per_block(const void* x, int dtype, const void* mean, int mean_group, int8_t* out, float* scale,
                         float sm_scale, int qmax, int blk, int B, int H, int S, int D,
                         const int64_t strides_x[3], const int64_t strides_out[3],
                         const void* rowdot_vec, int rowdot_group, float* rowdot_out, void* stream) {
  QuantCall c = quant_call("lbfa_quant_per_block", dense(x, strides_x), dense(out, strides_out), scale, dtype, mean, mean_group, sm_scale,
                           qmax, blk, B, H, S, D, D);
  c.rowdot_vec = rowdot_vec; c.rowdot_group = rowdot_group; c.rowdot_out = rowdot_out;
  if (int st = check_quant(c)) return st;
  return run_quant(c, (hipStream_t)stream);
}

// packed batch with the reference's scale layout [sum_blocks, H]
int lbfa_quant_per_block_varlen(const void* x, int dtype, const void* mean, int mean_group, int8_t* out, float* scale,
                                const int32_t* cu_seqlens, const int32_t* cu_seqlens_scale, float sm_scale, int qmax,
                                int blk, int B, int max_seqlen, int H, int D, const int64_t strides_x[2],
                                const int64_t strides_out[2], void* stream) {
  const char* who = "lbfa_quant_per_block_varlen";
  if (!cu_seqlens_scale) return fail(LBFA_EINVAL, "%s: null pointer", who);
  QuantCall c = quant_call(who, packed(x, strides_x), packed(out, strides_out), scale, dtype, mean, mean_group, sm_scale, qmax, blk, B, H,
                           max_seqlen, D, D);
  c.is_packed = true; c.cu_seqlens = cu_seqlens; c.cu_scale = cu_seqlens_scale;
  if (int st = check_quant(c)) return st;
  return run_quant(c, (hipStream_t)stream);
}

size_t lbfa_v_fp8_bytes(int B, int H, int S, int D) {
  if (B <= 0 || H <= 0 || S <= 0 || D <= 0) return 0;
  // payload [B,H,ceil(S/64),D,64] + fp32 amax scratch [B,H,D]
  return lbfa::v_fp8_payload_bytes(B, H, S, D) + (size_t)B * H * D * sizeof(float);
}

int lbfa_quant_v_fp8(const void* v, int dtype, uint8_t* v_fp8, float* v_scale, int B, int H, int S, int D,
                     const int64_t strides_v[3], void* stream) {
  const Operand t = dense(v, strides_v);
  if (int st = check_v_fp8(t, dtype, v_fp8, v_scale, B, H, S, D)) return st;
  return run_v_fp8(t, dtype, v_fp8, v_scale, B, H, S, D, D, (hipStream_t)stream);
}

int lbfa_cast_bf16_to_f16(const void* src, void* dst, int B, int H, int S, int D, const int64_t strides_src[3],
                          const int64_t strides_dst[3], void* stream) {
  const Operand s = dense(src, strides_src), d = dense(dst, strides_dst);
  if (!s.p || !d.p) return fail(LBFA_EINVAL, "lbfa_cast_bf16_to_f16: null pointer");
  if (B <= 0 || H <= 0 || S <= 0 || D <= 0 || D % 8 != 0) return fail(LBFA_EINVAL, "lbfa_cast_bf16_to_f16: bad shape (D must be a multiple of 8)");
  if (!aligned(s, 16, 8) || !aligned(d, 16, 8))
    return fail(LBFA_EINVAL, "lbfa_cast_bf16_to_f16: tensors must be 16-byte aligned, strides multiples of 8 elements");
  g_err[0] = 0;
  return check_hip(lbfa::launch_cast_bf16_f16(src, dst, B, H, S, D, s.st, d.st, (hipStream_t)stream), "lbfa_cast_bf16_to_f16 launch");
}

int lbfa_attn_fwd(const int8_t* q, const int8_t* k, const void* v, int v_dtype, void* o, int o_dtype, float* lse,
                  const float* q_scale, const float* k_scale, const float* v_scale,
                  int B, int Hq, int Hkv, int Sq, int Sk, int D,
                  const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3],
                  const int64_t strides_o[3], int is_causal, void* stream) {
  const char* who = "lbfa_attn_fwd";
  const bool fp8 = v_dtype == LBFA_E4M3;
  const Shape s = dense_shape(B, Hq, Hkv, Sq, Sk, D);
  const Operand tq = dense(q, strides_q), tk = dense(k, strides_k), to = dense(o, strides_o);
  const Operand tv = fp8 || !strides_v ? Operand{v, {0, 0, 0}} : dense(v, strides_v);  // e4m3 V has no strides
  if (!tq.p || !tk.p || !v || !to.p || !q_scale || !k_scale) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (s.empty()) return fail(LBFA_EINVAL, "%s: empty tensor", who);
  if (int st = check_head_dim(D, false)) return st;
  if (int st = check_gqa(Hq, Hkv)) return st;
  if (v_dtype == LBFA_BF16)
    return fail(LBFA_EINVAL, "%s: v must be float16 (cast bfloat16 with lbfa_cast_bf16_to_f16, the `v.to(float16)` of the reference) or e4m3", who);
  if (v_dtype != LBFA_F16 && !fp8) return fail(LBFA_EINVAL, "%s: bad v_dtype %d", who, v_dtype);
  if (o_dtype != LBFA_F16 && o_dtype != LBFA_BF16) return fail(LBFA_EINVAL, "%s: bad o_dtype %d", who, o_dtype);
  if (fp8 && !v_scale) return fail(LBFA_EINVAL, "%s: v_scale is required for fp8 V", who);
  if (!fp8 && !strides_v) return fail(LBFA_EINVAL, "%s: strides_v is required for fp16 V", who);
  if (int st = check_causal(is_causal, Sq, Sk)) return st;
  if (!aligned(q, 16) || !aligned(k, 16) || !aligned(v, 16) || !aligned(o, 8))
    return fail(LBFA_EINVAL, "%s: q/k/v must be 16-byte aligned and o 8-byte aligned", who);
  if (!tq.strides_multiple_of(16) || !tk.strides_multiple_of(16)) return fail(LBFA_EINVAL, "%s: q/k strides must be multiples of 16 elements", who);
  if (!tv.strides_multiple_of(8)) return fail(LBFA_EINVAL, "%s: v strides must be multiples of 8 elements", who);
  if (!to.strides_multiple_of(4)) return fail(LBFA_EINVAL, "%s: o strides must be multiples of 4 elements", who);
  if (!window_ok(Sq, kAheadQ, tq.st[2], 1, D) || !window_ok(Sk, kAheadK, tk.st[2], 1, D) ||
      !(fp8 ? fp8_v_window_ok(Sk, D) : window_ok(Sk, kAheadK, tv.st[2], 2, D)))
    return fail(LBFA_EINVAL, "%s: per-(batch,head) operand window exceeds 2 GiB (seq stride x length too large)", who);
  if (int st = check_attn_grid(who, s)) return st;
  const lbfa::AttnParams p = attn_params(s, tq, tk, tv, to, q_scale, k_scale, v_scale, lse);
  return check_hip(launch_attention(AttnKernel::kCodes, p, D, v_dtype, o_dtype, is_causal ? 1 : 0, (hipStream_t)stream), "lbfa_attn_fwd launch");
}


// ---------------------------------------------------------------------------------------------------------------
// whole operator in one call
// ---------------------------------------------------------------------------------------------------------------
size_t lbfa_forward_workspace_bytes_dt(int B, int Hq, int Hkv, int Sq, int Sk, int D, int dtype, int pv_fp8, int smooth_k, int return_lse) {
  const Shape s = dense_shape(B, Hq, Hkv, Sq, Sk, D);
  return s.empty() || !head_dim_ok(D) ? 0 : fwd_layout(s, pv_fp8, dtype).total;  // whatever smooth_k and return_lse
}
size_t lbfa_forward_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Sk, int D, int pv_fp8, int smooth_k, int return_lse) {
  return lbfa_forward_workspace_bytes_dt(B, Hq, Hkv, Sq, Sk, D, LBFA_BF16, pv_fp8, smooth_k, return_lse);  // enough for either dtype
}

namespace {
// casts a bf16 V into its fp16 workspace copy, which is laid out as the K codes are
int run_v_cast(const char* what, const Shape& s, const Operand& v, const Operand& v16, hipStream_t stream) {
  return check_hip(lbfa::launch_cast_bf16_f16(v.p, const_cast<void*>(v16.p), s.mean_batch(), s.Hkv, s.mean_rows(), s.Dg, v.st, v16.st, stream), what);
}
}  // namespace

// The dense and the packed one-call forward are two bodies over the same stages (mean -> K quantiser -> V fp8 | V cast ->
// attention): their checks and messages differ line by line, and only this one has fp8 PV and the fused mean finalize.
int lbfa_forward(const void* q, const void* k, const void* v, int dtype, void* o, float* lse, void* workspace,
                 size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int Sk, int D,
                 const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3],
                 const int64_t strides_o[3], double sm_scale, int q_qmax, int k_qmax, int pv_fp8, int is_causal,
                 int smooth_k, void* stream_) {
  const char* who = "lbfa_forward";
  const hipStream_t stream = (hipStream_t)stream_;
  const Shape s = dense_shape(B, Hq, Hkv, Sq, Sk, D);  // s.D is what the kernels run on; channels >= D are never read or written
  const Operand tq = dense(q, strides_q), tk = dense(k, strides_k), tv = dense(v, strides_v), to = dense(o, strides_o);
  if (!tq.p || !tk.p || !tv.p || !to.p || !workspace) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (s.empty()) return fail(LBFA_EINVAL, "%s: empty tensor", who);
  if (int st = check_head_dim(D, true)) return st;
  if (int st = check_gqa(Hq, Hkv)) return st;
  const FwdLayout L = fwd_layout(s, pv_fp8, dtype);
  if (int st = check_workspace(who, workspace, workspace_bytes, L.total)) return st;
  if (int st = check_dtype(dtype)) return st;
  if (int st = check_qmax(who, "q_qmax", q_qmax)) return st;
  if (int st = check_qmax(who, "k_qmax", k_qmax)) return st;
  if (int st = check_input16(who, "q", tq)) return st;
  if (int st = check_input16(who, "k", tk)) return st;
  if (int st = check_input16(who, "v", tv)) return st;
  if (!aligned(to, 8, 4)) return fail(LBFA_EINVAL, "%s: o must be 8-byte aligned with strides that are multiples of 4 elements", who);
  if (int st = check_causal(is_causal, Sq, Sk)) return st;
  // Q is read as 16-bit elements, the K codes lie in the workspace with seq stride D
  if (!window_ok(Sq, kAheadQ, tq.st[2], 2, s.D) || !window_ok(Sk, kAheadK, s.D, 1, s.D) ||
      !(pv_fp8 ? fp8_v_window_ok(Sk, s.D) : window_ok(Sk, kAheadK, tv.st[2], 2, s.D)))
    return fail(LBFA_EINVAL, "%s: per-(batch,head) operand window exceeds 2 GiB", who);
  if (int st = check_attn_grid(who, s)) return st;
  char* ws = (char*)workspace;
  void* km = smooth_k ? (void*)(ws + L.km) : nullptr;
  float* ks = (float*)(ws + L.ks);
  uint8_t* v8 = (uint8_t*)(ws + L.v8);
  float* vs = (float*)(ws + L.vs);
  // smooth-K mean: fp64 partial sums per 256 / 1024 rows, and - while there are few of them - no separate finalize launch:
  // the K quantiser's workgroups add the partials of their (batch, head) themselves (same order, same roundings) and
  // store km for the LSE correction.  (mean_finalize alone is 6.6 us of pure launch latency at C2.)
  const int nsplit = (Sk + lbfa::mean_rows_per_split(Sk) - 1) / lbfa::mean_rows_per_split(Sk);
  const bool fuse_finalize = smooth_k && nsplit <= 64;
  const MeanCall mean = k_mean_call(s, tk, dtype, km, ws + L.part, !fuse_finalize);
  QuantCall kq = workspace_quant_call(nullptr, s, false, tk, dtype, km, ws + L.k8, ks, 1.0f, k_qmax);
  kq.mean_partial = fuse_finalize ? (const double*)(ws + L.part) : nullptr;
  kq.mean_nsplit = nsplit;
  if (smooth_k)
    if (int st = check_mean(mean)) return st;
  if (int st = check_quant(kq)) return st;
  if (pv_fp8)
    if (int st = check_v_fp8(tv, dtype, v8, vs, B, Hkv, Sk, s.D)) return st;

  if (smooth_k)
    if (int st = run_mean(mean, stream)) return st;
  if (int st = run_quant(kq, stream)) return st;
  Operand v_in = tv;
  int v_dtype = dtype;
  if (pv_fp8) {
    if (int st = run_v_fp8(tv, dtype, v8, vs, B, Hkv, Sk, s.D, D, stream)) return st;
    v_in = Operand{v8, {0, 0, 0}};
    v_dtype = LBFA_E4M3;
  } else if (v_cast_prepass(dtype, pv_fp8)) {
    v_in = s.contiguous(ws + L.v16, Hkv, Sk);
    if (int st = run_v_cast("lbfa_forward (V cast) launch", s, tv, v_in, stream)) return st;
    v_dtype = LBFA_F16;
  }
  // attention, with the LSE fix-up of src/core.py:344-350 fused into the epilogue
  lbfa::AttnParams p = attn_params(s, tq, kq.out, v_in, to, nullptr, ks, pv_fp8 ? vs : nullptr, lse);
  natural_log_lse(p, sm_scale);
  quantise_q_in_kernel(p, sm_scale, q_qmax, lse && smooth_k ? km : nullptr);
  return check_hip(launch_attention(AttnKernel::kQuantiseQ, p, s.D, v_dtype, dtype, is_causal ? 1 : 0, stream), "lbfa_forward launch");
}


// ---------------------------------------------------------------------------------------------------------------
// un-quantised attention: the FP16 branch of the precision router (src/core.py:1066-1096 -> default_attn, :46-69)
// ---------------------------------------------------------------------------------------------------------------
int lbfa_sdpa_fwd(const void* q, const void* k, const void* v, int dtype, void* o, float* lse,
                  int B, int Hq, int Hkv, int Sq, int Sk, int D,
                  const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3],
                  const int64_t strides_o[3], double sm_scale, int is_causal, void* stream) {
  const char* who = "lbfa_sdpa_fwd";
  const Shape s = dense_shape(B, Hq, Hkv, Sq, Sk, D);
  const Operand tq = dense(q, strides_q), tk = dense(k, strides_k), tv = dense(v, strides_v), to = dense(o, strides_o);
  if (!tq.p || !tk.p || !tv.p || !to.p) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (s.empty()) return fail(LBFA_EINVAL, "%s: empty tensor", who);
  if (int st = check_head_dim(D, true)) return st;
  if (int st = check_gqa(Hq, Hkv)) return st;
  if (int st = check_dtype(dtype)) return st;
  if (int st = check_causal(is_causal, Sq, Sk)) return st;
  if (!(sm_scale > 0.0)) return fail(LBFA_EINVAL, "%s: sm_scale must be positive (the row maximum is tracked on the unscaled scores)", who);
  if (!aligned(q, 16) || !aligned(k, 16) || !aligned(v, 16) || !aligned(o, 8))
    return fail(LBFA_EINVAL, "%s: q/k/v must be 16-byte aligned and o 8-byte aligned", who);
  if (!tq.strides_multiple_of(8) || !tk.strides_multiple_of(8) || !tv.strides_multiple_of(8))
    return fail(LBFA_EINVAL, "%s: q/k/v strides must be multiples of 8 elements", who);
  if (!to.strides_multiple_of(4)) return fail(LBFA_EINVAL, "%s: o strides must be multiples of 4 elements", who);
  // the windows count the head dim as given
  if (!window_ok(Sq, kAheadQ, tq.st[2], 2, D) || !window_ok(Sk, kAheadK, tk.st[2], 2, D) || !window_ok(Sk, kAheadK, tv.st[2], 2, D))
    return fail(LBFA_EINVAL, "%s: per-(batch,head) operand window exceeds 2 GiB", who);
  if (int st = check_attn_grid(who, s)) return st;
  lbfa::AttnParams p = attn_params(s, tq, tk, tv, to, nullptr, nullptr, nullptr, lse);
  natural_log_lse(p, 0.0);
  p.qk_scale = (float)(sm_scale * 1.44269504);
  return check_hip(launch_attention(AttnKernel::kF16, p, s.D, dtype, dtype, is_causal ? 1 : 0, (hipStream_t)stream), "lbfa_sdpa_fwd launch");
}

// ---------------------------------------------------------------------------------------------------------------
// packed variable-length batches (reference: sageattn_varlen, src/core.py:356-491)
// ---------------------------------------------------------------------------------------------------------------
namespace {
// the attention stage of a packed batch: Q as int8 codes with q_scale, or (quantise_q) as fp16 / bf16 for the in-kernel quantiser
struct PackedAttnCall {
  Shape s;
  Operand q, k, v, o;
  int v_dtype, o_dtype;
  const float *q_scale, *k_scale;
  const int32_t *cu_qscale, *cu_kscale;  // the reference's packed scale tables, or both null: padded [B,H,max_blocks]
  bool quantise_q;
  int q_qmax;
};
int check_packed_attn(const char* who, const PackedAttnCall& c) {
  const Shape& s = c.s;
  if (!c.q.p || !c.k.p || !c.v.p || !c.o.p || (!c.q_scale && !c.quantise_q) || !c.k_scale || !s.cu_q || !s.cu_k)
    return fail(LBFA_EINVAL, "%s: null pointer", who);
  if ((c.cu_qscale == nullptr) != (c.cu_kscale == nullptr)) return fail(LBFA_EINVAL, "%s: give both scale offset tables or neither", who);
  if (s.empty()) return fail(LBFA_EINVAL, "%s: empty batch", who);
  if (int st = check_head_dim(c.quantise_q ? s.D : s.Dg, false)) return st;  // codes come with the head dim the kernels run on
  if (int st = check_gqa(s.Hq, s.Hkv)) return st;
  if (c.v_dtype != LBFA_F16) return fail(LBFA_EINVAL, "%s: v must be float16 (cast bfloat16 with lbfa_cast_bf16_to_f16)", who);
  if (c.o_dtype != LBFA_F16 && c.o_dtype != LBFA_BF16) return fail(LBFA_EINVAL, "%s: bad o_dtype %d", who, c.o_dtype);
  if (!aligned(c.q.p, 16) || !aligned(c.k.p, 16) || !aligned(c.v.p, 16) || !aligned(c.o.p, 8))
    return fail(LBFA_EINVAL, "%s: q/k/v must be 16-byte aligned and o 8-byte aligned", who);
  if (!(c.quantise_q || c.q.strides_multiple_of(16)) || !c.k.strides_multiple_of(16))
    return fail(LBFA_EINVAL, "%s: q/k strides must be multiples of 16 elements", who);
  if (c.quantise_q && !c.q.strides_multiple_of(8)) return fail(LBFA_EINVAL, "%s: q strides must be multiples of 8 elements", who);
  if (c.quantise_q)
    if (int st = check_qmax(who, "q_qmax", c.q_qmax)) return st;
  if (!c.v.strides_multiple_of(8)) return fail(LBFA_EINVAL, "%s: v strides must be multiples of 8 elements", who);
  if (!c.o.strides_multiple_of(4)) return fail(LBFA_EINVAL, "%s: o strides must be multiples of 4 elements", who);
  if (!window_ok(s.Sq, kAheadQ, c.q.st[2], c.quantise_q ? 2 : 1, s.D) || !window_ok(s.Sk, kAheadK, c.k.st[2], 1, s.D) ||
      !window_ok(s.Sk, kAheadK, c.v.st[2], 2, s.D))
    return fail(LBFA_EINVAL, "%s: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)", who);
  return check_attn_grid(who, s);
}
lbfa::AttnParams packed_attn_params(const PackedAttnCall& c) {
  lbfa::AttnParams p = attn_params(c.s, c.q, c.k, c.v, c.o, c.q_scale, c.k_scale, nullptr, nullptr);
  if (c.cu_qscale) {
    p.qsc_b = c.s.Hq; p.qsc_h = 1; p.qsc_blk = c.s.Hq;      // [sum_q_blocks, Hq]  (attn_qk_int8_block_varlen.py:134-138)
    p.ksc_b = c.s.Hkv; p.ksc_h = 1; p.ksc_blk = c.s.Hkv;    // [sum_k_blocks, Hkv]
  }
  p.cu_qscale = c.cu_qscale; p.cu_kscale = c.cu_kscale;
  return p;
}
}  // namespace

int lbfa_attn_fwd_varlen(const int8_t* q, const int8_t* k, const void* v, int v_dtype, void* o, int o_dtype,
                         const float* q_scale, const float* k_scale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                         const int32_t* cu_seqlens_q_scale, const int32_t* cu_seqlens_k_scale,
                         int B, int Hq, int Hkv, int max_seqlen_q, int max_seqlen_k, int D,
                         const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                         const int64_t strides_o[2], int is_causal, void* stream) {
  const char* who = "lbfa_attn_fwd_varlen";
  if (!cu_seqlens_q_scale || !cu_seqlens_k_scale) return fail(LBFA_EINVAL, "%s: null pointer", who);
  const PackedAttnCall c{packed_shape(B, Hq, Hkv, 0, 0, max_seqlen_q, max_seqlen_k, D, cu_seqlens_q, cu_seqlens_k),
                   packed(q, strides_q), packed(k, strides_k), packed(v, strides_v), packed(o, strides_o), v_dtype, o_dtype,
                   q_scale, k_scale, cu_seqlens_q_scale, cu_seqlens_k_scale, false, 127};
  if (int st = check_packed_attn(who, c)) return st;
  const lbfa::AttnParams p = packed_attn_params(c);
  return check_hip(launch_attention(AttnKernel::kCodes, p, D, v_dtype, o_dtype, is_causal ? 1 : 0, (hipStream_t)stream), who);
}

size_t lbfa_forward_varlen_workspace_bytes_dt(int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q,
                                              int max_seqlen_k, int D, int dtype) {
  const Shape s = packed_shape(B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, nullptr, nullptr);
  return s.empty() || total_q <= 0 || total_k <= 0 || !head_dim_ok(D) ? 0 : fwd_layout(s, 0, dtype).total;
}
size_t lbfa_forward_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q,
                                           int max_seqlen_k, int D) {
  return lbfa_forward_varlen_workspace_bytes_dt(B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, LBFA_BF16);  // enough for either dtype
}

namespace {
int forward_varlen_impl(const char* who, const void* q, const void* k, const void* v, int dtype, void* o, float* lse,
                        const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, void* workspace, size_t workspace_bytes,
                        int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D,
                        const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                        const int64_t strides_o[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                        hipStream_t stream) {
  const Shape s = packed_shape(B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, cu_seqlens_q, cu_seqlens_k);
  const Operand tq = packed(q, strides_q), tk = packed(k, strides_k), tv = packed(v, strides_v), to = packed(o, strides_o);
  if (!tq.p || !tk.p || !tv.p || !to.p || !workspace || !cu_seqlens_q || !cu_seqlens_k) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (s.empty() || total_q <= 0 || total_k <= 0) return fail(LBFA_EINVAL, "%s: empty batch", who);
  if (int st = check_head_dim(D, true)) return st;
  if (int st = check_gqa(Hq, Hkv)) return st;
  const FwdLayout L = fwd_layout(s, 0, dtype);
  if (int st = check_workspace(who, workspace, workspace_bytes, L.total)) return st;
  if (int st = check_dtype(dtype)) return st;
  if (int st = check_qmax(who, "q_qmax", q_qmax)) return st;
  if (int st = check_qmax(who, "k_qmax", k_qmax)) return st;
  if (!aligned(q, 16) || !aligned(k, 16) || !aligned(v, 16) || !aligned(o, 8))
    return fail(LBFA_EINVAL, "%s: q/k/v must be 16-byte aligned and o 8-byte aligned", who);
  if (!tq.strides_multiple_of(8) || !tk.strides_multiple_of(8) || !tv.strides_multiple_of(8))
    return fail(LBFA_EINVAL, "%s: q / k / v strides must be multiples of 8 elements", who);
  if (!to.strides_multiple_of(4)) return fail(LBFA_EINVAL, "%s: o strides must be multiples of 4 elements", who);
  // Q is read as 16-bit elements, the K codes lie in the workspace with token stride Hkv * D
  if (!window_ok(s.Sq, kAheadQ, tq.st[2], 2, s.D) || !window_ok(s.Sk, kAheadK, (int64_t)Hkv * s.D, 1, s.D) ||
      !window_ok(s.Sk, kAheadK, tv.st[2], 2, s.D))
    return fail(LBFA_EINVAL, "%s: per-sequence operand window exceeds 2 GiB (token stride x max_seqlen too large)", who);
  if (int st = check_attn_grid(who, s)) return st;
  char* ws = (char*)workspace;
  void* km = smooth_k ? (void*)(ws + L.km) : nullptr;
  float* ks = (float*)(ws + L.ks);
  const bool cast_v = v_cast_prepass(dtype, 0);
  const MeanCall mean = k_mean_call(s, tk, dtype, km, ws + L.part, true);
  const QuantCall kq = workspace_quant_call("lbfa_forward_varlen (K)", s, false, tk, dtype, km, ws + L.k8, ks, 1.0f, k_qmax);
  // Q is quantised by the attention kernel itself (blocks restart at every sequence start, as the quantiser's do)
  const PackedAttnCall attn{s, tq, kq.out, cast_v ? s.contiguous(ws + L.v16, Hkv, s.Sk) : tv, to, LBFA_F16, dtype, nullptr, ks,
                            nullptr, nullptr, true, q_qmax};
  if (smooth_k)
    if (int st = check_mean(mean)) return st;
  if (int st = check_quant(kq)) return st;
  if (int st = check_packed_attn(who, attn)) return st;

  if (smooth_k)
    if (int st = run_mean(mean, stream)) return st;
  if (int st = run_quant(kq, stream)) return st;
  if (cast_v)
    if (int st = run_v_cast("lbfa_forward_varlen (V cast) launch", s, tv, attn.v, stream)) return st;
  lbfa::AttnParams p = packed_attn_params(attn);
  // the mean reaches the attention kernel only for the LSE correction: without an LSE this is the call of lbfa_forward_varlen
  quantise_q_in_kernel(p, sm_scale, q_qmax, lse ? km : nullptr);
  if (lse) {  // [Hq, total_q] natural-log LSE with the smooth-K correction formed in the kernel (the q_dot_vec of lbfa_forward)
    p.lse = lse;
    p.lse_hs = total_q;
    natural_log_lse(p, sm_scale);
  }
  return check_hip(launch_attention(AttnKernel::kQuantiseQ, p, s.D, LBFA_F16, dtype, is_causal ? 1 : 0, stream), who);
}
}  // namespace

int lbfa_forward_varlen(const void* q, const void* k, const void* v, int dtype, void* o,
                        const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, void* workspace, size_t workspace_bytes,
                        int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D,
                        const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                        const int64_t strides_o[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                        void* stream) {
  return forward_varlen_impl("lbfa_forward_varlen", q, k, v, dtype, o, nullptr, cu_seqlens_q, cu_seqlens_k, workspace,
                             workspace_bytes, B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, strides_q, strides_k,
                             strides_v, strides_o, sm_scale, q_qmax, k_qmax, is_causal, smooth_k, (hipStream_t)stream);
}

int lbfa_forward_varlen_lse(const void* q, const void* k, const void* v, int dtype, void* o, float* lse,
                            const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, void* workspace, size_t workspace_bytes,
                            int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D,
                            const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2],
                            const int64_t strides_o[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                            void* stream) {
  if (!aligned(lse, 4)) return fail(LBFA_EINVAL, "lbfa_forward_varlen_lse: lse must be 4-byte aligned");
  return forward_varlen_impl("lbfa_forward_varlen_lse", q, k, v, dtype, o, lse, cu_seqlens_q, cu_seqlens_k, workspace,
                             workspace_bytes, B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, strides_q, strides_k,
                             strides_v, strides_o, sm_scale, q_qmax, k_qmax, is_causal, smooth_k, (hipStream_t)stream);
}


// ---------------------------------------------------------------------------------------------------------------
// backward (attn_bwd.hip): straight-through on the quantiser, deterministic two-kernel FlashAttention-2 form
// ---------------------------------------------------------------------------------------------------------------
namespace {
// in: q, k, v, o, dout; grad: dq, dk, dv.  Dense and packed differ by the descriptions alone, and in that the dense operator
// admits q_qmax = k_qmax = 0 (un-quantised scores) and requires Sq == Sk when causal.
int backward_impl(const char* who, const Shape& s, const Operand (&in)[5], const Operand (&grad)[3], int dtype, const float* lse,
                  const float* dlse, void* workspace, size_t workspace_bytes, double sm_scale, int q_qmax, int k_qmax,
                  int is_causal, int smooth_k, hipStream_t stream) {
  for (const Operand& t : in)
    if (!t.p) return fail(LBFA_EINVAL, "%s: null pointer", who);
  for (const Operand& t : grad)
    if (!t.p) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (!lse || !workspace || (s.is_packed && (!s.cu_q || !s.cu_k))) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (s.is_packed ? s.empty() || s.total_q <= 0 || s.total_k <= 0 : s.empty())
    return fail(LBFA_EINVAL, "%s: empty %s", who, s.is_packed ? "batch" : "tensor");
  if (s.Dg != 64 && s.Dg != 128) return fail(LBFA_EINVAL, "%s: Unsupported head_dim: %d (64 or 128; pad other head dims with zeros)", who, s.Dg);
  if (int st = check_gqa(s.Hq, s.Hkv)) return st;
  if (int st = check_dtype(dtype)) return st;
  const auto int_range = [](int qmax) { return qmax == 7 || qmax == 127; };
  if (s.is_packed) {
    if (!int_range(q_qmax) || !int_range(k_qmax)) return fail(LBFA_EINVAL, "%s: q_qmax / k_qmax must each be 127 or 7, got %d / %d", who, q_qmax, k_qmax);
  } else {
    if (!(q_qmax == 0 && k_qmax == 0) && !(int_range(q_qmax) && int_range(k_qmax)))
      return fail(LBFA_EINVAL, "%s: q_qmax / k_qmax must both be 0 (un-quantised) or each 127 / 7, got %d / %d", who, q_qmax, k_qmax);
    if (int st = check_causal(is_causal, s.Sq, s.Sk)) return st;  // a packed batch masks each sequence by its own lengths
  }
  if (!(sm_scale > 0.0)) return fail(LBFA_EINVAL, "%s: sm_scale must be positive", who);
  const char* names[5] = {"q", "k", "v", "o", "dout"};
  for (int i = 0; i < 5; ++i)
    if (int st = check_input16(who, names[i], in[i])) return st;
  if (!aligned(grad[0].p, 2) || !aligned(grad[1].p, 2) || !aligned(grad[2].p, 2)) return fail(LBFA_EINVAL, "%s: dq / dk / dv must be 2-byte aligned", who);
  if (!aligned(lse, 4) || !aligned(dlse, 4)) return fail(LBFA_EINVAL, "%s: lse / dlse must be 4-byte aligned", who);
  const bool quant = q_qmax != 0, sm = quant && smooth_k;
  const BwdLayout L = bwd_layout(s, quant, smooth_k);
  if (int st = check_workspace(who, workspace, workspace_bytes, L.total)) return st;
  const int nkb = (s.Sk + 63) / 64, nqb = (s.Sq + 63) / 64;
  const bool rows_fit = s.is_packed ? (int64_t)s.Hq * s.total_q + (int64_t)s.Hkv * s.total_k <= 0x7fffffffLL - 255
                                    : (int64_t)s.B * s.Hq * s.Sq <= 0x7fffffffLL;
  if (!rows_fit || (int64_t)s.B * s.Hq * nqb > 0x7fffffffLL || (int64_t)s.B * s.Hkv * nkb > 0x7fffffffLL)
    return fail(LBFA_EINVAL, "%s: grid too large", who);

  // The forward's codes, bit for bit: the same mean and quantiser kernels.  The one-call forward quantises Q inside its attention
  // kernel with this arithmetic (128-row blocks, sm_scale * log2(e) folded in; packed: restarting at every sequence, lengths
  // cut at max_seqlen_q) and may fuse the last step of the mean into the K quantiser, in the same order.  The smooth-K
  // correction q . km is formed by the pre-pass in the forward kernels' order (bwd_prep_kernel), not here.
  char* ws = (char*)workspace;
  void* km = sm ? (void*)(ws + L.km) : nullptr;
  float *qs = (float*)(ws + L.qs), *ks = (float*)(ws + L.ks);
  const MeanCall mean = k_mean_call(s, in[1], dtype, km, ws + L.part, true);
  const QuantCall kq = workspace_quant_call("lbfa_backward_varlen (K)", s, false, in[1], dtype, km, ws + L.k8, ks, 1.0f, k_qmax);
  const QuantCall qq = workspace_quant_call("lbfa_backward_varlen (Q)", s, true, in[0], dtype, nullptr, ws + L.q8, qs,
                                            (float)(sm_scale * 1.44269504), q_qmax);
  if (sm)
    if (int st = check_mean(mean)) return st;
  if (quant) {
    if (int st = check_quant(kq)) return st;
    if (int st = check_quant(qq)) return st;
  }

  lbfa::BwdParams p = bwd_params(s, in, grad, lse, dlse, (float*)(ws + L.lse2), (float*)(ws + L.delta), sm_scale);
  if (quant) {
    if (sm)
      if (int st = run_mean(mean, stream)) return st;
    if (int st = run_quant(kq, stream)) return st;
    if (int st = run_quant(qq, stream)) return st;
    p.q8 = (const int8_t*)qq.out.p; p.k8 = (const int8_t*)kq.out.p;
    p.q_scale = qs; p.k_scale = ks;
    p.km = (const unsigned short*)km;
    p.q8b = qq.out.st[0]; p.q8h = qq.out.st[1]; p.q8s = qq.out.st[2];
    p.k8b = kq.out.st[0]; p.k8h = kq.out.st[1]; p.k8s = kq.out.st[2];
  }
  g_err[0] = 0;
  return check_hip(lbfa::launch_attn_bwd(p, dtype, quant, is_causal != 0, stream), s.is_packed ? "lbfa_backward_varlen launch" : "lbfa_backward launch");
}
}  // namespace

size_t lbfa_backward_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Sk, int D, int q_qmax, int smooth_k) {
  const Shape s = dense_shape(B, Hq, Hkv, Sq, Sk, D);
  return s.empty() || (D != 64 && D != 128) ? 0 : bwd_layout(s, q_qmax != 0, smooth_k).total;
}

int lbfa_backward(const void* q, const void* k, const void* v, const void* o, const void* dout, int dtype, const float* lse,
                  const float* dlse, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                  int B, int Hq, int Hkv, int Sq, int Sk, int D,
                  const int64_t strides_q[3], const int64_t strides_k[3], const int64_t strides_v[3], const int64_t strides_o[3],
                  const int64_t strides_dout[3], const int64_t strides_dq[3], const int64_t strides_dk[3],
                  const int64_t strides_dv[3], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                  void* stream) {
  const Operand in[5] = {dense(q, strides_q), dense(k, strides_k), dense(v, strides_v), dense(o, strides_o), dense(dout, strides_dout)};
  const Operand grad[3] = {dense(dq, strides_dq), dense(dk, strides_dk), dense(dv, strides_dv)};
  return backward_impl("lbfa_backward", dense_shape(B, Hq, Hkv, Sq, Sk, D), in, grad, dtype, lse, dlse, workspace, workspace_bytes,
                       sm_scale, q_qmax, k_qmax, is_causal, smooth_k, (hipStream_t)stream);
}

size_t lbfa_backward_varlen_workspace_bytes(int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                                            int D, int q_qmax, int smooth_k) {
  const Shape s = packed_shape(B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, nullptr, nullptr);
  if (s.empty() || total_q <= 0 || total_k <= 0 || (D != 64 && D != 128) || (q_qmax != 127 && q_qmax != 7)) return 0;
  return bwd_layout(s, true, smooth_k).total;
}

int lbfa_backward_varlen(const void* q, const void* k, const void* v, const void* o, const void* dout, int dtype, const float* lse,
                         const float* dlse, void* dq, void* dk, void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                         void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int total_q, int total_k,
                         int max_seqlen_q, int max_seqlen_k, int D,
                         const int64_t strides_q[2], const int64_t strides_k[2], const int64_t strides_v[2], const int64_t strides_o[2],
                         const int64_t strides_dout[2], const int64_t strides_dq[2], const int64_t strides_dk[2],
                         const int64_t strides_dv[2], double sm_scale, int q_qmax, int k_qmax, int is_causal, int smooth_k,
                         void* stream) {
  const Operand in[5] = {packed(q, strides_q), packed(k, strides_k), packed(v, strides_v), packed(o, strides_o), packed(dout, strides_dout)};
  const Operand grad[3] = {packed(dq, strides_dq), packed(dk, strides_dk), packed(dv, strides_dv)};
  return backward_impl("lbfa_backward_varlen", packed_shape(B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D, cu_seqlens_q, cu_seqlens_k),
                       in, grad, dtype, lse, dlse, workspace, workspace_bytes, sm_scale, q_qmax, k_qmax, is_causal, smooth_k,
                       (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// int8 KV cache and split-KV decode attention (kvcache.hip, attn_decode.hip, attn_prefill.hip), over a contiguous cache
// [B, Hkv, capacity, D] or a pool of pages behind a block table, V as fp16 or as e4m3 codes with a scale per key, the K codes a
// byte each or - the _k4 entry points - two to a byte.
// An append and a cache read (decode or cached prefill) are described once each, AppendCall and ReadCall: one set of checks in one
// order, one fill of the parameter block, one launch.  An entry point is ONE statement: it names itself and its parameter block
// and passes its arguments in the order of its signature - the pool arguments as paged(...), v_scale beside v_cache, q_lens beside
// seqlens.  The block is the whole choice: what the call is (paged, fp8 V, packed K, prefill), which fields are filled and which kernel
// runs all follow from its type (lbfa::CacheBlock), so the three cannot disagree.
// ---------------------------------------------------------------------------------------------------------------
}  // extern "C": the templates and overloads of this section need C++ linkage

namespace {
constexpr int kDecodeMaxRows = 64;     // query rows per kv head one decode workgroup serves
constexpr int kDecodeWaves = 1024;     // workgroups (one wave each) that fill the part: 256 CUs x 4 SIMDs
constexpr int kDecodeMinTiles = 4;     // no key slice shorter than 4 tiles of 64 keys
constexpr int kDecodeMaxSplits = 256;
constexpr int64_t kPrefillMaxGridX = (1 << 24) - 1;  // x extent of the prefill and combine grids (256 threads each)
constexpr int kPrefillGroups = 512;    // four-wave workgroups that fill the part: 256 CUs x 2

// Where the keys live.  Contiguous: the capacity.  Paged: the pool; check_pool sets cap = max_pages * page_size.
struct Pool {
  int cap;  // the most keys a sequence can hold
  lbfa::PoolParams at;
};
Pool contiguous(int capacity) { return Pool{capacity, {}}; }
Pool paged(const int32_t* block_table, const int32_t* slots, int num_slots, int num_pages, int page_size, int max_pages_per_seq) {
  lbfa::PoolParams at{};
  at.block_table = block_table; at.slots = slots;
  at.num_slots = num_slots; at.num_pages = num_pages; at.page_size = page_size; at.max_pages = max_pages_per_seq;
  return Pool{0, at};
}
int check_pool(const char* who, int B, bool paged, Pool& k) {
  const lbfa::PoolParams& a = k.at;
  if (!paged)
    return k.cap > 0 && k.cap % LBFA_BLKK == 0 ? 0 : fail(LBFA_EINVAL, "%s: capacity must be a positive multiple of 64, got %d", who, k.cap);
  if (a.page_size <= 0 || a.page_size % LBFA_BLKK != 0)
    return fail(LBFA_EINVAL, "%s: page_size must be a positive multiple of 64, got %d", who, a.page_size);
  if (a.num_pages < 1 || a.num_slots < 1 || a.max_pages < 1)
    return fail(LBFA_EINVAL, "%s: num_pages, num_slots and max_pages_per_seq must be at least 1, got %d, %d and %d", who, a.num_pages,
                a.num_slots, a.max_pages);
  if ((int64_t)a.max_pages * a.page_size > 0x7fffffffLL)
    return fail(LBFA_EINVAL, "%s: max_pages_per_seq * page_size must stay below 2^31 keys", who);
  if (B > a.num_slots) return fail(LBFA_EINVAL, "%s: B (%d) exceeds num_slots (%d)", who, B, a.num_slots);
  k.cap = a.max_pages * a.page_size;
  return 0;
}
bool pool_aligned(const Pool& k) { return aligned(k.at.block_table, 4) && aligned(k.at.slots, 4); }

// V of the cache: fp16 rows {v_cache}, or - the _v8 entry points - e4m3 codes and one fp32 scale per key {v_cache, v_scale}
struct CachedV {
  const void* p;
  const float* scale = nullptr;
};
// the sequence lengths of a read: {seqlens}, a cached prefill adds its ragged query lengths {seqlens, q_lens}
struct Lens {
  const int32_t* seqlens;
  const int32_t* q_lens = nullptr;
};

// what the append entry points state, in the order of their signatures
struct AppendCall {
  const char* who;
  Operand k_new, v_new;
  int dtype;
  const int32_t* new_lens;
  const void* km;
  int8_t* k_codes;
  float* k_scale;
  CachedV v;
  void* k_tail;
  const int32_t* seqlens;
  int B, Hkv, T, D;
  Pool pool;
  int k_qmax;
  bool paged, v8, k4;  // what the parameter block is
};
int check_append(AppendCall& c) {
  const char* who = c.who;
  if (!c.k_new.p || !c.v_new.p || !c.k_codes || !c.k_scale || !c.v.p || !c.k_tail || !c.seqlens || (c.paged && !c.pool.at.block_table) ||
      (c.v8 && !c.v.scale))
    return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (c.B <= 0 || c.Hkv <= 0 || c.T <= 0) return fail(LBFA_EINVAL, "%s: empty tensor", who);
  if (int st = check_head_dim(c.D, false)) return st;
  if (int st = check_pool(who, c.B, c.paged, c.pool)) return st;
  if (int st = check_dtype(c.dtype)) return st;
  if (int st = check_qmax(who, "k_qmax", c.k_qmax)) return st;
  if (c.k4 && c.k_qmax != 7) return fail(LBFA_EINVAL, "%s: k_qmax must be 7 (the codes of a nibble-packed cache take 4 bits), got %d", who, c.k_qmax);
  if (int st = check_input16(who, "k_new", c.k_new)) return st;
  if (int st = check_input16(who, "v_new", c.v_new)) return st;
  if (!aligned(c.k_codes, 16) || !aligned(c.v.p, 16) || !aligned(c.k_tail, 16) || !aligned(c.km, 16) || !aligned(c.k_scale, 4) ||
      !aligned(c.seqlens, 4) || !aligned(c.new_lens, 4) || !pool_aligned(c.pool))
    return fail(LBFA_EINVAL, "%s: cache tensors and km must be 16-byte aligned, k_scale / seqlens / new_lens%s 4-byte aligned", who,
                c.paged ? " / block_table / slots" : "");
  if (c.v8 && !aligned(c.v.scale, 16)) return fail(LBFA_EINVAL, "%s: v_scale must be 16-byte aligned", who);
  if (c.B > 65535 || c.Hkv > 65535) return fail(LBFA_EINVAL, "%s: grid too large", who);
  return 0;
}
void fill(lbfa::AppendParams& p, const AppendCall& c) {
  p.k_new = (const unsigned short*)c.k_new.p; p.v_new = (const unsigned short*)c.v_new.p;
  p.new_lens = c.new_lens; p.km = (const unsigned short*)c.km;
  p.k_codes = c.k_codes; p.k_scale = c.k_scale; p.v = (unsigned short*)const_cast<void*>(c.v.p); p.k_tail = (unsigned short*)c.k_tail;
  p.seqlens = c.seqlens;
  p.kb = c.k_new.st[0]; p.kh = c.k_new.st[1]; p.ks = c.k_new.st[2];
  p.vb = c.v_new.st[0]; p.vh = c.v_new.st[1]; p.vs = c.v_new.st[2];
  p.B = c.B; p.Hkv = c.Hkv; p.T = c.T; p.cap = c.pool.cap;
  p.qmax = (float)c.k_qmax;
}

// what the decode and the cached-prefill entry points state, in the order of their signatures
struct ReadCall {
  const char* who;
  Operand q, o;
  int dtype;
  const int8_t* k_codes;
  const float* k_scale;
  CachedV v;
  const void* km;
  const int32_t *seqlens, *q_lens;
  float* lse;
  void* workspace;
  size_t workspace_bytes;
  int B, Hq, Hkv, Sq, D;
  Pool pool;
  int max_seqlen_k, num_splits;
  double sm_scale;
  int q_qmax, is_causal;
  bool paged, v8, prefill;  // what the parameter block is
  int splits;               // set by check_decode: num_splits, or the split rule's choice
};
int check_decode(ReadCall& c) {
  const char* who = c.who;
  if (!c.q.p || !c.o.p || !c.k_codes || !c.k_scale || !c.v.p || !c.seqlens || (c.paged && !c.pool.at.block_table) ||
      (c.v8 && !c.v.scale))
    return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (c.B <= 0 || c.Hq <= 0 || c.Hkv <= 0 || c.Sq <= 0) return fail(LBFA_EINVAL, "%s: empty tensor", who);
  if (int st = check_head_dim(c.D, false)) return st;
  if (int st = check_gqa(c.Hq, c.Hkv)) return st;
  const int64_t M = (int64_t)c.Sq * (c.Hq / c.Hkv);
  if (!c.prefill && M > kDecodeMaxRows)
    return fail(LBFA_EINVAL, "%s: Sq * (Hq / Hkv) = %lld query rows per kv head, the limit is %d (longer queries belong on the dense operator)",
                who, (long long)M, kDecodeMaxRows);
  if (int st = check_pool(who, c.B, c.paged, c.pool)) return st;
  if (c.max_seqlen_k < 1 || c.max_seqlen_k > c.pool.cap)
    return c.paged ? fail(LBFA_EINVAL, "%s: max_seqlen_k must be in [1, max_pages_per_seq * page_size], got %d (limit %d)", who,
                          c.max_seqlen_k, c.pool.cap)
                   : fail(LBFA_EINVAL, "%s: max_seqlen_k must be in [1, capacity], got %d (capacity %d)", who, c.max_seqlen_k, c.pool.cap);
  if (c.num_splits < 0 || c.num_splits > 65535)
    return fail(LBFA_EINVAL, "%s: num_splits must be in [0, 65535] (0: chosen by %s), got %d", who,
                c.prefill ? "lbfa_prefill_num_splits" : "lbfa_decode_num_splits", c.num_splits);
  if (int st = check_dtype(c.dtype)) return st;
  if (int st = check_qmax(who, "q_qmax", c.q_qmax)) return st;
  if (!(c.sm_scale > 0.0)) return fail(LBFA_EINVAL, "%s: sm_scale must be positive", who);
  if (int st = check_input16(who, "q", c.q)) return st;
  if (!aligned(c.o, 8, 4)) return fail(LBFA_EINVAL, "%s: o must be 8-byte aligned with strides that are multiples of 4 elements", who);
  if (!aligned(c.k_codes, 16) || !aligned(c.v.p, 16) || !aligned(c.km, 16) || !aligned(c.k_scale, 4) || !aligned(c.seqlens, 4) ||
      !pool_aligned(c.pool) || !aligned(c.lse, 4) || !aligned(c.q_lens, 4))
    return fail(LBFA_EINVAL, "%s: cache tensors and km must be 16-byte aligned, k_scale / seqlens%s%s / lse 4-byte aligned", who,
                c.prefill ? " / q_lens" : "", c.paged ? " / block_table / slots" : "");
  if (c.v8 && !aligned(c.v.scale, 16)) return fail(LBFA_EINVAL, "%s: v_scale must be 16-byte aligned", who);
  if (c.prefill) c.splits = c.num_splits ? c.num_splits : lbfa_prefill_num_splits(c.B, c.Hq, c.Sq, c.max_seqlen_k);
  else c.splits = c.num_splits ? c.num_splits : lbfa_decode_num_splits(c.B, c.Hkv, c.max_seqlen_k);
  // prefill: grid (Q blocks x slices, Hq, B) of 256 threads, the combine's (M, Hkv, B) of 256: a launch whose gridDim.x * blockDim.x
  // reaches 2^32 is refused by the runtime, and the combine is the SECOND launch - so both are bounded here, before the first
  if (c.prefill && (c.Hq > 65535 || M > kPrefillMaxGridX || ((int64_t)c.Sq + LBFA_BLKQ - 1) / LBFA_BLKQ * c.splits > kPrefillMaxGridX))
    return fail(LBFA_EINVAL, "%s: grid too large (Sq * (Hq / Hkv) and ceil(Sq / 128) * num_splits must stay below 2^24, Hq below 65536)", who);
  // (the partials of both operators have the same size: one row per query row and slice)
  if (const size_t need = lbfa_decode_workspace_bytes(c.B, c.Hq, c.Hkv, c.Sq, c.D, c.max_seqlen_k, c.splits)) {
    if (int st = check_workspace(who, c.workspace, c.workspace_bytes, need)) return st;
    if (!c.workspace) return fail(LBFA_EINVAL, "%s: null pointer", who);
  }
  if (c.B > 65535 || c.Hkv > 65535) return fail(LBFA_EINVAL, "%s: grid too large", who);
  return 0;
}
void fill(lbfa::DecodeParams& p, const ReadCall& c) {
  const int M = c.Sq * (c.Hq / c.Hkv);
  p.q = (const unsigned short*)c.q.p; p.k_codes = c.k_codes; p.k_scale = c.k_scale; p.v = (const unsigned short*)c.v.p;
  p.km = c.lse ? (const unsigned short*)c.km : nullptr;  // km only enters the LSE correction
  p.seqlens = c.seqlens; p.o = const_cast<void*>(c.o.p); p.lse = c.lse;
  p.qb = c.q.st[0]; p.qh = c.q.st[1]; p.qs = c.q.st[2];
  p.ob = c.o.st[0]; p.oh = c.o.st[1]; p.os = c.o.st[2];
  p.B = c.B; p.Hq = c.Hq; p.Hkv = c.Hkv; p.Sq = c.Sq; p.group = c.Hq / c.Hkv; p.M = M;
  p.cap = c.pool.cap; p.max_k = c.max_seqlen_k; p.splits = c.splits; p.causal = c.is_causal ? 1 : 0;
  p.q_sm_scale = (float)(c.sm_scale * 1.44269504);  // ONE rounding of the double product, as lbfa_forward
  p.q_qmax = (float)c.q_qmax;
  p.corr_scale = (float)c.sm_scale;
  if (c.splits > 1) {
    const size_t rows = (size_t)c.B * c.Hkv * c.splits * (size_t)M;
    p.ws_acc = (float*)c.workspace;
    p.ws_ml = (float*)((char*)c.workspace + align256(rows * c.D * sizeof(float)));
  }
}

// The parameter block P of a checked call: the AppendParams / DecodeParams every block starts with, then what P adds to them - the
// pool, the scales of the fp8 V cache, the prefill fields - by what P is.
template <class P, class Call>
P block_of(const Call& c) {
  using Is = lbfa::CacheBlock<P>;
  P p{};
  fill(p, c);
  if constexpr (std::is_base_of<lbfa::PoolParams, P>::value) {
    lbfa::PoolParams& at = p;
    at = c.pool.at;
  }
  if constexpr (Is::v_bits == 8) p.v_scale = const_cast<decltype(p.v_scale)>(c.v.scale);
  if constexpr (Is::op == lbfa::CacheOp::kPrefill) {
    p.nQ = (c.Sq + LBFA_BLKQ - 1) / LBFA_BLKQ;
    p.q_lens = c.q_lens;
  }
  return p;
}
int check_launch(hipError_t e, const char* who) {
  return e == hipSuccess ? LBFA_OK : fail(LBFA_ELAUNCH, "%s launch: %s", who, hipGetErrorString(e));
}

// an append into the cache that P describes
template <class P>
int run_append(const char* who, const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km, int8_t* k_codes,
               float* k_scale, CachedV v, void* k_tail, const int32_t* seqlens, int B, int Hkv, int T, int D, const Pool& pool,
               const int64_t strides_k[3], const int64_t strides_v[3], int k_qmax, void* stream) {
  using Is = lbfa::CacheBlock<P>;
  static_assert(Is::op == lbfa::CacheOp::kAppend, "run_append takes the parameter block of an append");
  AppendCall c{who, dense(k_new, strides_k), dense(v_new, strides_v), dtype, new_lens, km, k_codes, k_scale, v, k_tail, seqlens,
               B, Hkv, T, D, pool, k_qmax, Is::paged, Is::v_bits == 8, Is::k_bits == 4};
  if (int st = check_append(c)) return st;
  const P p = block_of<P>(c);
  g_err[0] = 0;
  return check_launch(lbfa::launch_append(p, dtype, D, (hipStream_t)stream), who);
}
// a decode or a cached prefill over the cache that P describes
template <class P>
int run_read(const char* who, const void* q, int dtype, const int8_t* k_codes, const float* k_scale, CachedV v, const void* km, Lens lens,
             void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, const Pool& pool,
             int max_seqlen_k, int num_splits, const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax,
             int is_causal, void* stream) {
  using Is = lbfa::CacheBlock<P>;
  static_assert(Is::op != lbfa::CacheOp::kAppend, "run_read takes the parameter block of a decode or a prefill");
  constexpr bool prefill = Is::op == lbfa::CacheOp::kPrefill;
  ReadCall c{who, dense(q, strides_q), dense(o, strides_o), dtype, k_codes, k_scale, v, km, lens.seqlens, lens.q_lens, lse, workspace,
             workspace_bytes, B, Hq, Hkv, Sq, D, pool, max_seqlen_k, num_splits, sm_scale, q_qmax, is_causal,
             Is::paged, Is::v_bits == 8, prefill, 0};
  if (int st = check_decode(c)) return st;
  const P p = block_of<P>(c);
  g_err[0] = 0;
  if constexpr (prefill) return check_launch(lbfa::launch_prefill(p, dtype, D, (hipStream_t)stream), who);
  else return check_launch(lbfa::launch_decode(p, dtype, D, (hipStream_t)stream), who);
}
// the parameter blocks of the fp8 V cache
template <class Base> using AppendV8 = lbfa::V8Params<Base, float*>;
template <class Base> using ReadV8 = lbfa::V8Params<Base, const float*>;
// the parameter blocks of the nibble-packed K cache: the sibling's block, k_codes two codes per byte behind the same pointer
template <class Base> using K4 = lbfa::K4Params<Base>;
int8_t* nibbles(uint8_t* k_codes) { return reinterpret_cast<int8_t*>(k_codes); }
const int8_t* nibbles(const uint8_t* k_codes) { return reinterpret_cast<const int8_t*>(k_codes); }
}  // namespace

extern "C" {

int lbfa_kvcache_mean(const void* k_new, int dtype, const int32_t* new_lens, void* km, int B, int Hkv, int T, int D,
                      const int64_t strides_k[3], void* stream) {
  const char* who = "lbfa_kvcache_mean";
  const Operand tk = dense(k_new, strides_k);
  if (!tk.p || !new_lens || !km) return fail(LBFA_EINVAL, "%s: null pointer", who);
  if (B <= 0 || Hkv <= 0 || T <= 0) return fail(LBFA_EINVAL, "%s: empty tensor", who);
  if (int st = check_head_dim(D, false)) return st;
  if (int st = check_dtype(dtype)) return st;
  if (int st = check_input16(who, "k_new", tk)) return st;
  if (B > 65535) return fail(LBFA_EINVAL, "%s: grid too large", who);
  lbfa::RaggedMeanParams p{};
  p.k_new = (const unsigned short*)k_new; p.new_lens = new_lens; p.km = (unsigned short*)km;
  p.kb = tk.st[0]; p.kh = tk.st[1]; p.ks = tk.st[2];
  p.Hkv = Hkv; p.T = T;
  g_err[0] = 0;
  return check_hip(lbfa::launch_kvcache_mean(p, dtype, B, D, (hipStream_t)stream), "lbfa_kvcache_mean launch");
}

int lbfa_kvcache_append(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                        int8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                        int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                        int k_qmax, void* stream) {
  return run_append<lbfa::AppendParams>("lbfa_kvcache_append", k_new, v_new, dtype, new_lens, km, k_codes, k_scale, {v_cache}, k_tail,
                                        seqlens, B, Hkv, T, D, contiguous(capacity), strides_k, strides_v, k_qmax, stream);
}

int lbfa_kvcache_paged_append(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                              int8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                              const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T, int D, int num_slots,
                              int num_pages, int page_size, int max_pages_per_seq, const int64_t strides_k[3],
                              const int64_t strides_v[3], int k_qmax, void* stream) {
  return run_append<lbfa::PagedAppendParams>("lbfa_kvcache_paged_append", k_new, v_new, dtype, new_lens, km, k_codes, k_scale, {v_cache},
                                             k_tail, seqlens, B, Hkv, T, D,
                                             paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq), strides_k,
                                             strides_v, k_qmax, stream);
}

// the fp8 V cache: the two appends above with v_cache as e4m3 codes and v_scale, one fp32 per key, behind it
int lbfa_kvcache_append_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                           int8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail, const int32_t* seqlens,
                           int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                           int k_qmax, void* stream) {
  return run_append<AppendV8<lbfa::AppendParams>>("lbfa_kvcache_append_v8", k_new, v_new, dtype, new_lens, km, k_codes, k_scale,
                                                  {v_cache, v_scale}, k_tail, seqlens, B, Hkv, T, D, contiguous(capacity), strides_k,
                                                  strides_v, k_qmax, stream);
}

int lbfa_kvcache_paged_append_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                                 int8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail,
                                 const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T,
                                 int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq,
                                 const int64_t strides_k[3], const int64_t strides_v[3], int k_qmax, void* stream) {
  return run_append<AppendV8<lbfa::PagedAppendParams>>("lbfa_kvcache_paged_append_v8", k_new, v_new, dtype, new_lens, km, k_codes,
                                                       k_scale, {v_cache, v_scale}, k_tail, seqlens, B, Hkv, T, D,
                                                       paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                                       strides_k, strides_v, k_qmax, stream);
}

// The split rule: as many key slices as it takes for B * Hkv * slices one-wave workgroups to reach 1024 (four per CU), but no
// slice shorter than 4 tiles of 64 keys (below that the per-slice prologue - Q quantiser, first-tile latency - and the
// partial results outweigh the parallelism), at most 256.  A pure function of its arguments.
int lbfa_decode_num_splits(int B, int Hkv, int max_seqlen_k) {
  if (B <= 0 || Hkv <= 0 || max_seqlen_k <= 0) return 1;
  const int64_t groups = (int64_t)B * Hkv, tiles = ((int64_t)max_seqlen_k + LBFA_BLKK - 1) / LBFA_BLKK;
  int64_t s = (kDecodeWaves + groups - 1) / groups;
  if (s > tiles / kDecodeMinTiles) s = tiles / kDecodeMinTiles;
  if (s > kDecodeMaxSplits) s = kDecodeMaxSplits;
  return s < 1 ? 1 : (int)s;
}

size_t lbfa_decode_workspace_bytes(int B, int Hq, int Hkv, int Sq, int D, int max_seqlen_k, int num_splits) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || (D != 64 && D != 128) || Hq % Hkv != 0 || num_splits < 0) return 0;
  const int splits = num_splits ? num_splits : lbfa_decode_num_splits(B, Hkv, max_seqlen_k);
  if (splits <= 1) return 0;  // one slice writes O itself
  const size_t rows = (size_t)B * Hkv * splits * ((size_t)Sq * (Hq / Hkv));
  Bump ws;
  ws.take(rows * D * sizeof(float));  // un-normalised partial O
  ws.take(rows * 4 * sizeof(float));  // m, l, q . km
  return ws.used;
}

int lbfa_decode(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<lbfa::DecodeParams>("lbfa_decode", q, dtype, k_codes, k_scale, {v_cache}, km, {seqlens}, o, lse, workspace,
                                      workspace_bytes, B, Hq, Hkv, Sq, D, contiguous(capacity), max_seqlen_k, num_splits, strides_q,
                                      strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_decode_paged(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                      const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, void* o, float* lse,
                      void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages,
                      int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                      const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<lbfa::PagedDecodeParams>("lbfa_decode_paged", q, dtype, k_codes, k_scale, {v_cache}, km, {seqlens}, o, lse,
                                           workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                           paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                           max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

// the fp8 V cache: the two decodes above with v_cache as e4m3 codes and v_scale, one fp32 per key, behind it
int lbfa_decode_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                   const void* km, const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                   int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                   const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<ReadV8<lbfa::DecodeParams>>("lbfa_decode_v8", q, dtype, k_codes, k_scale, {v_cache, v_scale}, km, {seqlens}, o,
                                              lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D, contiguous(capacity),
                                              max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_decode_paged_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                         const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* block_table,
                         const int32_t* slots, void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv,
                         int Sq, int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k,
                         int num_splits, const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax,
                         int is_causal, void* stream) {
  return run_read<ReadV8<lbfa::PagedDecodeParams>>("lbfa_decode_paged_v8", q, dtype, k_codes, k_scale, {v_cache, v_scale}, km,
                                                   {seqlens}, o, lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                                   paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                                   max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal,
                                                   stream);
}

// The split rule of the cached prefill: as many key slices as it takes for B * Hq * ceil(Sq / 128) four-wave workgroups to reach
// 512 (two per CU, the analogue of decode's four one-wave ones), no slice shorter than 4 tiles of 64 keys, at most 256.
int lbfa_prefill_num_splits(int B, int Hq, int Sq, int max_seqlen_k) {
  if (B <= 0 || Hq <= 0 || Sq <= 0 || max_seqlen_k <= 0) return 1;
  const int64_t groups = (int64_t)B * Hq * (((int64_t)Sq + LBFA_BLKQ - 1) / LBFA_BLKQ);
  const int64_t tiles = ((int64_t)max_seqlen_k + LBFA_BLKK - 1) / LBFA_BLKK;
  int64_t s = (kPrefillGroups + groups - 1) / groups;
  if (s > tiles / kDecodeMinTiles) s = tiles / kDecodeMinTiles;
  if (s > kDecodeMaxSplits) s = kDecodeMaxSplits;
  return s < 1 ? 1 : (int)s;
}

size_t lbfa_prefill_workspace_bytes(int B, int Hq, int Hkv, int Sq, int D, int max_seqlen_k, int num_splits) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || num_splits < 0) return 0;
  const int splits = num_splits ? num_splits : lbfa_prefill_num_splits(B, Hq, Sq, max_seqlen_k);
  return lbfa_decode_workspace_bytes(B, Hq, Hkv, Sq, D, max_seqlen_k, splits);  // the decode kernel's partials
}

int lbfa_prefill(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                 const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                 int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                 const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<lbfa::PrefillParams>("lbfa_prefill", q, dtype, k_codes, k_scale, {v_cache}, km, {seqlens, q_lens}, o, lse,
                                       workspace, workspace_bytes, B, Hq, Hkv, Sq, D, contiguous(capacity), max_seqlen_k,
                                       num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_prefill_paged(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                       const int32_t* seqlens, const int32_t* q_lens, const int32_t* block_table, const int32_t* slots, void* o,
                       float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots,
                       int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits,
                       const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal,
                       void* stream) {
  return run_read<lbfa::PagedPrefillParams>("lbfa_prefill_paged", q, dtype, k_codes, k_scale, {v_cache}, km, {seqlens, q_lens}, o,
                                            lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                            paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                            max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

// the fp8 V cache: the two cached prefills above with v_cache as e4m3 codes and v_scale, one fp32 per key, behind it
int lbfa_prefill_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                    const void* km, const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace,
                    size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                    const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<ReadV8<lbfa::PrefillParams>>("lbfa_prefill_v8", q, dtype, k_codes, k_scale, {v_cache, v_scale}, km,
                                               {seqlens, q_lens}, o, lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                               contiguous(capacity), max_seqlen_k, num_splits, strides_q, strides_o, sm_scale,
                                               q_qmax, is_causal, stream);
}

int lbfa_prefill_paged_v8(const void* q, int dtype, const int8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                          const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* q_lens,
                          const int32_t* block_table, const int32_t* slots, void* o, float* lse, void* workspace,
                          size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages, int page_size,
                          int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                          const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<ReadV8<lbfa::PagedPrefillParams>>("lbfa_prefill_paged_v8", q, dtype, k_codes, k_scale, {v_cache, v_scale}, km,
                                                    {seqlens, q_lens}, o, lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                                    paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                                    max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal,
                                                    stream);
}

// The nibble-packed K cache: every entry point above once more with k_codes as two codes per byte (uint8 [.., key, D / 2]: byte j
// of a row holds channel 2 j in bits 0..3 and channel 2 j + 1 in bits 4..7).  Each is its sibling's statement over K4<block> with
// k_codes passed as the bytes they are; an append takes k_qmax 7 only.
int lbfa_kvcache_append_k4(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                           uint8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                           int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                           int k_qmax, void* stream) {
  return run_append<K4<lbfa::AppendParams>>("lbfa_kvcache_append_k4", k_new, v_new, dtype, new_lens, km, nibbles(k_codes), k_scale, {v_cache}, k_tail,
                                        seqlens, B, Hkv, T, D, contiguous(capacity), strides_k, strides_v, k_qmax, stream);
}

int lbfa_kvcache_paged_append_k4(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                                 uint8_t* k_codes, float* k_scale, void* v_cache, void* k_tail, const int32_t* seqlens,
                                 const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T, int D, int num_slots,
                                 int num_pages, int page_size, int max_pages_per_seq, const int64_t strides_k[3],
                                 const int64_t strides_v[3], int k_qmax, void* stream) {
  return run_append<K4<lbfa::PagedAppendParams>>("lbfa_kvcache_paged_append_k4", k_new, v_new, dtype, new_lens, km, nibbles(k_codes), k_scale, {v_cache},
                                             k_tail, seqlens, B, Hkv, T, D,
                                             paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq), strides_k,
                                             strides_v, k_qmax, stream);
}

int lbfa_kvcache_append_k4_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                              uint8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail, const int32_t* seqlens,
                              int B, int Hkv, int T, int D, int capacity, const int64_t strides_k[3], const int64_t strides_v[3],
                              int k_qmax, void* stream) {
  return run_append<K4<AppendV8<lbfa::AppendParams>>>("lbfa_kvcache_append_k4_v8", k_new, v_new, dtype, new_lens, km, nibbles(k_codes), k_scale,
                                                  {v_cache, v_scale}, k_tail, seqlens, B, Hkv, T, D, contiguous(capacity), strides_k,
                                                  strides_v, k_qmax, stream);
}

int lbfa_kvcache_paged_append_k4_v8(const void* k_new, const void* v_new, int dtype, const int32_t* new_lens, const void* km,
                                    uint8_t* k_codes, float* k_scale, uint8_t* v_cache, float* v_scale, void* k_tail,
                                    const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, int B, int Hkv, int T,
                                    int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq,
                                    const int64_t strides_k[3], const int64_t strides_v[3], int k_qmax, void* stream) {
  return run_append<K4<AppendV8<lbfa::PagedAppendParams>>>("lbfa_kvcache_paged_append_k4_v8", k_new, v_new, dtype, new_lens, km, nibbles(k_codes),
                                                       k_scale, {v_cache, v_scale}, k_tail, seqlens, B, Hkv, T, D,
                                                       paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                                       strides_k, strides_v, k_qmax, stream);
}

int lbfa_decode_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                   const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                   int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                   const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<K4<lbfa::DecodeParams>>("lbfa_decode_k4", q, dtype, nibbles(k_codes), k_scale, {v_cache}, km, {seqlens}, o, lse, workspace,
                                      workspace_bytes, B, Hq, Hkv, Sq, D, contiguous(capacity), max_seqlen_k, num_splits, strides_q,
                                      strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_decode_paged_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                         const int32_t* seqlens, const int32_t* block_table, const int32_t* slots, void* o, float* lse,
                         void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages,
                         int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                         const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<K4<lbfa::PagedDecodeParams>>("lbfa_decode_paged_k4", q, dtype, nibbles(k_codes), k_scale, {v_cache}, km, {seqlens}, o, lse,
                                           workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                           paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                           max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_decode_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                      const void* km, const int32_t* seqlens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                      int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                      const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<K4<ReadV8<lbfa::DecodeParams>>>("lbfa_decode_k4_v8", q, dtype, nibbles(k_codes), k_scale, {v_cache, v_scale}, km, {seqlens}, o,
                                              lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D, contiguous(capacity),
                                              max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_decode_paged_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                            const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* block_table,
                            const int32_t* slots, void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv,
                            int Sq, int D, int num_slots, int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k,
                            int num_splits, const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax,
                            int is_causal, void* stream) {
  return run_read<K4<ReadV8<lbfa::PagedDecodeParams>>>("lbfa_decode_paged_k4_v8", q, dtype, nibbles(k_codes), k_scale, {v_cache, v_scale}, km,
                                                   {seqlens}, o, lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                                   paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                                   max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal,
                                                   stream);
}

int lbfa_prefill_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                    const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace, size_t workspace_bytes,
                    int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                    const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<K4<lbfa::PrefillParams>>("lbfa_prefill_k4", q, dtype, nibbles(k_codes), k_scale, {v_cache}, km, {seqlens, q_lens}, o, lse,
                                       workspace, workspace_bytes, B, Hq, Hkv, Sq, D, contiguous(capacity), max_seqlen_k,
                                       num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_prefill_paged_k4(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const void* v_cache, const void* km,
                          const int32_t* seqlens, const int32_t* q_lens, const int32_t* block_table, const int32_t* slots, void* o,
                          float* lse, void* workspace, size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots,
                          int num_pages, int page_size, int max_pages_per_seq, int max_seqlen_k, int num_splits,
                          const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal,
                          void* stream) {
  return run_read<K4<lbfa::PagedPrefillParams>>("lbfa_prefill_paged_k4", q, dtype, nibbles(k_codes), k_scale, {v_cache}, km, {seqlens, q_lens}, o,
                                            lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                            paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                            max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal, stream);
}

int lbfa_prefill_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache, const float* v_scale,
                       const void* km, const int32_t* seqlens, const int32_t* q_lens, void* o, float* lse, void* workspace,
                       size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int capacity, int max_seqlen_k, int num_splits,
                       const int64_t strides_q[3], const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<K4<ReadV8<lbfa::PrefillParams>>>("lbfa_prefill_k4_v8", q, dtype, nibbles(k_codes), k_scale, {v_cache, v_scale}, km,
                                               {seqlens, q_lens}, o, lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                               contiguous(capacity), max_seqlen_k, num_splits, strides_q, strides_o, sm_scale,
                                               q_qmax, is_causal, stream);
}

int lbfa_prefill_paged_k4_v8(const void* q, int dtype, const uint8_t* k_codes, const float* k_scale, const uint8_t* v_cache,
                             const float* v_scale, const void* km, const int32_t* seqlens, const int32_t* q_lens,
                             const int32_t* block_table, const int32_t* slots, void* o, float* lse, void* workspace,
                             size_t workspace_bytes, int B, int Hq, int Hkv, int Sq, int D, int num_slots, int num_pages, int page_size,
                             int max_pages_per_seq, int max_seqlen_k, int num_splits, const int64_t strides_q[3],
                             const int64_t strides_o[3], double sm_scale, int q_qmax, int is_causal, void* stream) {
  return run_read<K4<ReadV8<lbfa::PagedPrefillParams>>>("lbfa_prefill_paged_k4_v8", q, dtype, nibbles(k_codes), k_scale, {v_cache, v_scale}, km,
                                                    {seqlens, q_lens}, o, lse, workspace, workspace_bytes, B, Hq, Hkv, Sq, D,
                                                    paged(block_table, slots, num_slots, num_pages, page_size, max_pages_per_seq),
                                                    max_seqlen_k, num_splits, strides_q, strides_o, sm_scale, q_qmax, is_causal,
                                                    stream);
}

}  // extern "C"
